#!/usr/bin/env python3
"""Single-shard location (shmr_ec_locate_batch_dev) against the parity check it
starts with, interleaved rounds in one process, HIP events around each leg, on
the clean RS(8,3) x 4 MiB x 512 batch of tools/verify_ab.py (bench.py's padded
slot layout, separate data / parity regions):

  a  verify        verify_batch_dev on clean codewords
  a2 verify        the same leg again: the run-to-run spread locate is held to
  b  locate        locate_batch_dev on the same clean batch (the common case of a
                   scrub: verify, the bitmap preset, one word per tile, resolve)
  c  locate_dmg    locate_batch_dev with one data shard of EVERY block replaced
                   by random bytes: every tile runs the syndrome and ratio math

Every leg is counted with verify's algorithmic bytes, (k + p) * len * B, so the
fractions of 8 TB/s compare as times do; leg c reads the data and parity twice.
The scratch and result arrays are allocated once (the raw C ABI call).  One
JSON line per leg.

    python tools/locate_ab.py [--out profiles/r08/locate_ab.jsonl]
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

HBM_PEAK = 8e12
K, P, MIB, BLOCKS = 8, 3, 4, 512


def slot(S):
    pitch = (S + 4095) // 4096 * 4096
    return pitch + 4096 if pitch % 65536 == 0 else pitch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--out", default="", help="also append the JSON lines to this file")
    a = ap.parse_args()
    import shmr_amd
    from shmr_amd import _native

    assert torch.cuda.is_available(), "locate_ab.py measures on the GPU"
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream()
    k, p, B = K, P, BLOCKS
    S = shmr_amd.calculate_shard_size(MIB << 20, k)
    pitch = slot(S)
    rs = shmr_amd.ReedSolomon(k, p)
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    data = torch.randint(0, 256, (B, k, pitch), dtype=torch.uint8, device=dev, generator=g)
    parity = torch.zeros((B, p, pitch), dtype=torch.uint8, device=dev)
    rs.encode_batch_dev(data, parity, shard_len=S)              # the clean codewords
    damaged = data.clone()
    damaged[:, 3, :S] = torch.randint(0, 256, (B, S), dtype=torch.uint8, device=dev, generator=g)
    words = torch.empty(B, dtype=torch.int32, device=dev)
    located = torch.empty(B, dtype=torch.int32, device=dev)
    work = torch.empty(rs.locate_work_size(B), dtype=torch.uint8, device=dev)
    v = ctypes.c_void_p
    L = _native.lib()

    def verify():
        rs.verify_batch_dev(data, parity, shard_len=S, out=words)

    def locate_of(d):
        def run():
            rc = L.shmr_ec_locate_batch_dev(rs._h, v(d.data_ptr()), pitch, k * pitch, v(parity.data_ptr()), pitch,
                                            p * pitch, B, S, v(words.data_ptr()), v(located.data_ptr()),
                                            v(work.data_ptr()), work.numel(), 0, v(st.cuda_stream))
            assert rc == 0, rc
        return run

    legs = {"a_verify": verify, "a2_verify": verify, "b_locate_clean": locate_of(data),
            "c_locate_damaged": locate_of(damaged)}
    for f in legs.values():
        for _ in range(a.warmup):
            f()
    torch.cuda.synchronize()
    # the answers before anything is timed
    legs["b_locate_clean"]()
    torch.cuda.synchronize()
    assert not words.cpu().numpy().any() and (located.cpu().numpy() == -1).all()
    legs["c_locate_damaged"]()
    torch.cuda.synchronize()
    assert (words.cpu().numpy() == (1 << p) - 1).all() and (located.cpu().numpy() == 3).all()
    times = {n: [] for n in legs}
    for _ in range(a.rounds):
        for n, f in legs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            for _ in range(a.iters):
                f()
            e1.record(st)
            torch.cuda.synchronize()
            times[n].append(e0.elapsed_time(e1) / a.iters)
    algo = (k + p) * S * B
    lines = []
    for n, ts in times.items():
        med = float(np.median(ts))
        lines.append(json.dumps({
            "leg": n, "k": k, "p": p, "block_mib": MIB, "blocks": B, "shard_len": S, "pitch": pitch,
            "ms_per_launch": round(med, 4), "ms_min": round(min(ts), 4), "ms_max": round(max(ts), 4),
            "ms_rounds": [round(t, 4) for t in ts],
            "bytes": algo, "frac_hbm_peak": round(algo / (med / 1e3) / HBM_PEAK, 4),
            "rounds": a.rounds, "iters": a.iters, "flavour": _native.flavour(),
            "build_id": L.shmr_ec_build_id().decode()}))
        print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
