#!/usr/bin/env python3
"""Checked reconstruct against the plain reconstruct, interleaved rounds in one
process, HIP events around each leg.  One [B, k + p, pitch] buffer of clean
codewords (shard slots of S rounded up to 4 KiB plus one 4 KiB page where that
is a multiple of 64 KiB, as bench.py pads them); the same data shard is absent
in every block (a failed drive: one pattern, one launch set per leg):

  a  reconstruct   reconstruct_batch_dev           reads k, writes e = 1 shard
  b  checked       reconstruct_checked_batch_dev   reads k + s, writes e
  c  check_only    ... with rebuild=False          reads k + s, writes nothing

s = p - 1 surplus shards.  Each leg is counted with its own algorithmic bytes;
`ratio_to_reconstruct` is the leg's time over leg a's in the same run, next to
the traffic model's (k + s + e) / (k + e) (leg c: (k + s) / (k + e)).  One JSON
line per leg and shape.

    python tools/check_ab.py [--out profiles/r08/check_ab.jsonl]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

SHAPES = [(8, 3, 4, 512), (10, 4, 16, 64)]      # k, p, block MiB, blocks
ABSENT = 3                                      # the data shard every block has lost


def slot(S):
    pitch = (S + 4095) // 4096 * 4096
    return pitch + 4096 if pitch % 65536 == 0 else pitch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default="", help="also append the JSON lines to this file")
    a = ap.parse_args()
    import shmr_amd
    from shmr_amd import _native

    assert torch.cuda.is_available(), "check_ab.py measures on the GPU"
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream()
    lines = []
    for k, p, mib, B in SHAPES:
        S = shmr_amd.calculate_shard_size(mib << 20, k)
        pitch = slot(S)
        rs = shmr_amd.ReedSolomon(k, p)
        g = torch.Generator(device=dev)
        g.manual_seed(7)
        shards = torch.randint(0, 256, (B, k + p, pitch), dtype=torch.uint8, device=dev, generator=g)
        rs.encode_batch_dev(shards[:, :k], shards[:, k:], shard_len=S)          # the clean codewords
        lost = shards[:, ABSENT, :S].clone()
        present = np.ones((B, k + p), np.uint8)
        present[:, ABSENT] = 0
        words = torch.empty(B, dtype=torch.int32, device=dev)
        e, s = 1, p - 1

        def reconstruct():
            rs.reconstruct_batch_dev(shards, present, shard_len=S)

        def checked():
            rs.reconstruct_checked_batch_dev(shards, present, shard_len=S, out=words)

        def check_only():
            rs.reconstruct_checked_batch_dev(shards, present, shard_len=S, rebuild=False, out=words)

        legs = {"a_reconstruct": (reconstruct, k + e), "b_checked": (checked, k + s + e),
                "c_check_only": (check_only, k + s)}
        # the legs agree before they are timed: the rebuilt shard, clean words, one damaged input
        for name, (f, _) in legs.items():
            shards[:, ABSENT].fill_(0xA5)
            words.fill_(-1)
            f()
            torch.cuda.synchronize()
            if f is not check_only:
                assert torch.equal(shards[:, ABSENT, :S], lost), name
            if f is not reconstruct:
                assert not words.cpu().numpy().any(), name
        shards[:, ABSENT, :S] = lost
        shards[B // 2, 0, S - 1] ^= 1
        for f in (checked, check_only):
            f()
            torch.cuda.synchronize()
            want = [rs.checked_rows(present[0]) if b == B // 2 else 0 for b in range(B)]
            assert words.cpu().numpy().view(np.uint32).tolist() == want
        shards[B // 2, 0, S - 1] ^= 1
        reconstruct()
        for f, _ in legs.values():
            for _ in range(a.warmup):
                f()
        torch.cuda.synchronize()
        times = {n: [] for n in legs}
        for _ in range(a.rounds):
            for n, (f, _) in legs.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(st)
                for _ in range(a.iters):
                    f()
                e1.record(st)
                torch.cuda.synchronize()
                times[n].append(e0.elapsed_time(e1) / a.iters)
        base = float(np.median(times["a_reconstruct"]))
        for n, ts in times.items():
            med = float(np.median(ts))
            algo = legs[n][1] * S * B
            lines.append(json.dumps({
                "leg": n, "k": k, "p": p, "block_mib": mib, "blocks": B, "shard_len": S, "pitch": pitch,
                "absent": ABSENT, "ms_per_call": round(med, 4), "ms_min": round(min(ts), 4),
                "ms_max": round(max(ts), 4), "bytes": algo, "gib_per_s": round(algo / (med / 1e3) / 2 ** 30, 1),
                "ratio_to_reconstruct": round(med / base, 4), "model_ratio": round(legs[n][1] / (k + e), 4),
                "rounds": a.rounds, "iters": a.iters, "flavour": _native.flavour(),
                "build_id": _native.lib().shmr_ec_build_id().decode()}))
            print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
