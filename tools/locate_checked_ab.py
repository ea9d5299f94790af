#!/usr/bin/env python3
"""Degraded locate and repair against the checked reconstruct, interleaved rounds
in one process.  One [B, k + p, pitch] buffer of codewords (shard slots as
bench.py pads them, tools/check_ab.py); the same data shards are absent in
every block (failed drives: one pattern):

  a  clean batch:    locate_checked_batch_dev  /  reconstruct_checked_batch_dev
  b  1 % damaged:    the same two calls, one input byte damaged in every 100th block
  c  repair:         reconstruct_repair_batch_dev on the damaged batch  /
                     reconstruct_checked_batch_dev + a stream wait + reconstruct_batch_dev
                     with the damaged shards marked absent as well + a stream wait
                     (what a caller who KNEW the damaged shards would run)

Legs a and b: HIP events around `iters` calls, the native calls with
preallocated results (no allocation inside the timed loop on either side).
Leg c: both sides block, so wall time around `iters` calls; every call of
either side is preceded by the same small kernel that puts the damage back.
`ratio`: the first call's time over the second's in the same run.  One JSON
line per leg and shape.

    python tools/locate_checked_ab.py [--out profiles/r12/locate_checked_ab.jsonl]
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

SHAPES = [(8, 3, 4, 512, (3,)), (10, 4, 4, 512, (3,)), (10, 4, 4, 512, (3, 7))]   # k, p, block MiB, blocks, absent


def slot(S):
    pitch = (S + 4095) // 4096 * 4096
    return pitch + 4096 if pitch % 65536 == 0 else pitch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=11)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default="", help="also append the JSON lines to this file")
    a = ap.parse_args()
    import shmr_amd
    from shmr_amd import _native

    assert torch.cuda.is_available(), "locate_checked_ab.py measures on the GPU"
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream()
    L = _native.lib()
    v = ctypes.c_void_p
    lines = []
    for k, p, mib, B, absent in SHAPES:
        S = shmr_amd.calculate_shard_size(mib << 20, k)
        pitch = slot(S)
        t = k + p
        rs = shmr_amd.ReedSolomon(k, p)
        g = torch.Generator(device=dev)
        g.manual_seed(7)
        shards = torch.randint(0, 256, (B, t, pitch), dtype=torch.uint8, device=dev, generator=g)
        rs.encode_batch_dev(shards[:, :k], shards[:, k:], shard_len=S)          # the clean codewords
        code = shards[:, :, :S].clone()
        present = np.ones((B, t), np.uint8)
        present[:, list(absent)] = 0
        s = p - len(absent)
        pr_ptr = present.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))
        words = torch.empty(B, dtype=torch.int32, device=dev)
        located = torch.empty(B, dtype=torch.int32, device=dev)
        work = torch.empty(rs.locate_work_size(B), dtype=torch.uint8, device=dev)
        # 1 % of the blocks: one byte of input shard 0, at a different column each
        hit = np.arange(0, B, 100)
        flat = shards.view(-1)
        idx = torch.tensor([b * t * pitch + (b * 4099) % S for b in hit], dtype=torch.int64, device=dev)
        bad = (flat[idx] ^ 0x41).clone()
        good = flat[idx].clone()
        known = present.copy()                                                  # leg c's baseline knows the damage
        known[hit, 0] = 0

        def locate():
            rc = L.shmr_ec_locate_checked_batch_dev(rs._h, v(shards.data_ptr()), pitch, t * pitch, pr_ptr, B, S, 0,
                                                    v(words.data_ptr()), v(located.data_ptr()), v(work.data_ptr()),
                                                    work.numel(), 0, v(st.cuda_stream))
            assert rc == 0, rc

        def checked():
            rs.reconstruct_checked_batch_dev(shards, present, shard_len=S, out=words)

        def repair():
            flat[idx] = bad
            return rs.reconstruct_repair_batch_dev(shards, present, shard_len=S)

        def known_repair():
            flat[idx] = bad
            rs.reconstruct_checked_batch_dev(shards, present, shard_len=S, out=words)
            torch.cuda.synchronize()
            rs.reconstruct_batch_dev(shards, known, shard_len=S)
            torch.cuda.synchronize()

        # the calls agree before they are timed
        mask = rs.checked_rows(present[0])
        locate()
        torch.cuda.synchronize()
        assert not words.cpu().numpy().any() and (located.cpu().numpy() == -1).all()
        assert torch.equal(shards[:, :, :S], code)
        flat[idx] = bad
        locate()
        torch.cuda.synchronize()
        want = np.full(B, -1, np.int32)
        want[hit] = 0
        assert located.cpu().numpy().tolist() == want.tolist()
        assert words.cpu().numpy().view(np.uint32)[hit].tolist() == [mask] * len(hit)
        got, counts = repair()
        assert got.tolist() == want.tolist() and counts == {"clean": B - len(hit), "repaired": len(hit),
                                                            "not_repairable": 0}, counts
        assert torch.equal(shards[:, :, :S], code)
        known_repair()
        assert torch.equal(shards[:, :, :S], code)

        def timed_events(f):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            for _ in range(a.iters):
                f()
            e1.record(st)
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / a.iters

        def timed_wall(f):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.iters):
                f()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3 / a.iters

        legs = [("a_clean", locate, checked, timed_events, good), ("b_damaged_1pct", locate, checked, timed_events, bad),
                ("c_repair", repair, known_repair, timed_wall, bad)]
        for name, f_new, f_base, timed, state in legs:
            flat[idx] = state
            for _ in range(a.warmup):
                f_new()
                f_base()
            torch.cuda.synchronize()
            t_new, t_base = [], []
            for _ in range(a.rounds):
                flat[idx] = state
                t_new.append(timed(f_new))
                flat[idx] = state
                t_base.append(timed(f_base))
            m_new, m_base = float(np.median(t_new)), float(np.median(t_base))
            lines.append(json.dumps({
                "leg": name, "k": k, "p": p, "block_mib": mib, "blocks": B, "shard_len": S, "pitch": pitch,
                "absent": list(absent), "surplus": s, "damaged_blocks": 0 if state is good else len(hit),
                "ms_new": round(m_new, 4), "ms_new_min": round(min(t_new), 4), "ms_new_max": round(max(t_new), 4),
                "ms_base": round(m_base, 4), "ms_base_min": round(min(t_base), 4), "ms_base_max": round(max(t_base), 4),
                "ratio": round(m_new / m_base, 4),
                "ratio_per_round_min": round(min(x / y for x, y in zip(t_new, t_base)), 4),
                "ratio_per_round_max": round(max(x / y for x, y in zip(t_new, t_base)), 4),
                "checked_gib_per_s": round((k + p) * S * B / (m_base / 1e3) / 2 ** 30, 1) if timed is timed_events else None,
                "rounds": a.rounds, "iters": a.iters, "flavour": _native.flavour(),
                "build_id": L.shmr_ec_build_id().decode()}))
            print(lines[-1], flush=True)
        flat[idx] = good
        del shards, code
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
