#!/usr/bin/env python3
"""Parity check (ReedSolomon::verify) against encode, interleaved rounds in
one process, HIP events around each leg, on bench.py's padded slot layout
(separate data / parity regions, shard slots of S rounded up to 4 KiB plus one
4 KiB page where that is a multiple of 64 KiB):

  a  encode     encode_batch_dev (reads k, writes p shards per block)
  b  verify     verify_batch_dev on clean codewords (reads k + p, writes nothing)
  c  enc+cmp    what a caller did before verify_batch_dev: encode_batch_dev
                into scratch parity, then a device compare of scratch and stored
                parity (torch.ne + any per block, preallocated outputs)
  b1 / b2       (--u-ab) leg b with 4 KiB / 8 KiB full tiles forced (tools
                build, knob encode.chunks = 1 / 2 around the verify calls only):
                the tile-size A/B behind kern::verify_chunks

Every leg is counted with the same algorithmic bytes, (k + p) * len * B -- what
the check itself needs -- so the fractions of 8 TB/s compare as times do; leg c
moves (k + 3p) * len * B and more for the compare's temporaries.  One JSON line
per leg and shape.

    python tools/verify_ab.py [--out profiles/r07/verify_ab.jsonl] [--u-ab]
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

HBM_PEAK = 8e12
SHAPES = [(8, 3, 4, 512), (10, 4, 16, 64)]      # k, p, block MiB, blocks


def slot(S):
    pitch = (S + 4095) // 4096 * 4096
    return pitch + 4096 if pitch % 65536 == 0 else pitch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--u-ab", action="store_true", help="add legs b1 / b2 (tools build: U = 1 / 2 full tiles)")
    ap.add_argument("--out", default="", help="also append the JSON lines to this file")
    a = ap.parse_args()
    if a.u_ab:
        os.environ["SHMR_EC_FLAVOUR"] = "tools"     # kernel knobs: the tools build
    import shmr_amd
    from shmr_amd import _native

    assert torch.cuda.is_available(), "verify_ab.py measures on the GPU"
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream()
    lines = []
    for k, p, mib, B in SHAPES:
        S = shmr_amd.calculate_shard_size(mib << 20, k)
        pitch = slot(S)
        rs = shmr_amd.ReedSolomon(k, p)
        g = torch.Generator(device=dev)
        g.manual_seed(7)
        data = torch.randint(0, 256, (B, k, pitch), dtype=torch.uint8, device=dev, generator=g)
        parity = torch.zeros((B, p, pitch), dtype=torch.uint8, device=dev)
        scratch = torch.zeros((B, p, pitch), dtype=torch.uint8, device=dev)
        ne = torch.empty((B, p * pitch), dtype=torch.bool, device=dev)
        bad = torch.empty(B, dtype=torch.bool, device=dev)
        words = torch.empty(B, dtype=torch.int32, device=dev)
        rs.encode_batch_dev(data, parity, shard_len=S)          # the clean codewords

        def encode():
            rs.encode_batch_dev(data, scratch, shard_len=S)

        def verify():
            rs.verify_batch_dev(data, parity, shard_len=S, out=words)

        def enc_cmp():
            rs.encode_batch_dev(data, scratch, shard_len=S)
            torch.ne(scratch.view(B, -1), parity.view(B, -1), out=ne)
            torch.any(ne, dim=1, out=bad)

        def verify_u(u):
            def run():
                shmr_amd.set_tuning(**{"encode.chunks": u})
                try:
                    rs.verify_batch_dev(data, parity, shard_len=S, out=words)
                finally:
                    shmr_amd.set_tuning(**{"encode.chunks": -2})
            return run

        legs = {"a_encode": encode, "b_verify": verify, "c_encode_compare": enc_cmp}
        if a.u_ab:
            legs["b1_verify_u1"], legs["b2_verify_u2"] = verify_u(1), verify_u(2)
        for f in legs.values():
            for _ in range(a.warmup):
                f()
        torch.cuda.synchronize()
        # the legs agree before they are timed: clean codewords, and one damaged block
        assert not words.cpu().numpy().any() and not bad.cpu().numpy().any()
        parity[B // 2, p - 1, S - 1] ^= 1
        for f in legs.values():
            f()
            torch.cuda.synchronize()
            if f is not encode:
                got = (bad if f is enc_cmp else words != 0).cpu().numpy()
                assert got.tolist() == [b == B // 2 for b in range(B)], got
        parity[B // 2, p - 1, S - 1] ^= 1
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
        for n, ts in times.items():
            med = float(np.median(ts))
            lines.append(json.dumps({
                "leg": n, "k": k, "p": p, "block_mib": mib, "blocks": B, "shard_len": S, "pitch": pitch,
                "ms_per_launch": round(med, 4), "ms_min": round(min(ts), 4), "ms_max": round(max(ts), 4),
                "bytes": algo, "frac_hbm_peak": round(algo / (med / 1e3) / HBM_PEAK, 4),
                "rounds": a.rounds, "iters": a.iters, "flavour": _native.flavour(),
                "build_id": _native.lib().shmr_ec_build_id().decode()}))
            print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
