#!/usr/bin/env python3
"""Two-shard location (shmr_ec_locate_pair_batch_dev) against the single-shard
location it starts with, interleaved rounds in one process, HIP events around
each leg, on RS(10,4) x 16 MiB x 64 blocks (bench.py's padded slot layout,
separate data / parity regions):

  a  locate         locate_batch_dev on clean codewords
  a2 locate         the same leg again: the run-to-run spread the pair call is held to
  b  pair_clean     locate_pair_batch_dev on the same clean batch: locate plus the
                    preset, the select launch and pair launches that find an empty
                    worklist
  c  pair_dmg_skip  locate_pair_batch_dev with two bytes of two data shards of
  d  pair_dmg_all   --damaged of the blocks changed, one in the first and one in
                    the last tile: knob pair_skip = 1 (a wave leaves out candidates
                    that are already cleared) and 0 (every candidate in every
                    damaged tile)

Legs c and d also report the time per damaged block over leg b.  The scratch
and result arrays are allocated once (the raw C ABI call).  One JSON line per
leg.

    python tools/locate_pair_ab.py [--out profiles/r15/locate_pair_ab.jsonl]
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

K, P, MIB, BLOCKS = 10, 4, 16, 64


def slot(S):
    pitch = (S + 4095) // 4096 * 4096
    return pitch + 4096 if pitch % 65536 == 0 else pitch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--damaged", type=int, default=8, help="blocks of legs c and d with a damaged pair")
    ap.add_argument("--out", default="", help="also append the JSON lines to this file")
    a = ap.parse_args()
    import shmr_amd
    from shmr_amd import _native

    assert torch.cuda.is_available(), "locate_pair_ab.py measures on the GPU"
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
    hit = list(range(0, B, B // a.damaged))[:a.damaged]
    for b in hit:
        damaged[b, 2, 100] ^= 0x41
        damaged[b, 7, S - 5] ^= 0x17
    words = torch.empty(B, dtype=torch.int32, device=dev)
    located = torch.empty(2 * B, dtype=torch.int32, device=dev)
    work = torch.empty(rs.locate_pair_work_size(B), dtype=torch.uint8, device=dev)
    v = ctypes.c_void_p
    L = _native.lib()

    def call(fn, d):
        rc = fn(rs._h, v(d.data_ptr()), pitch, k * pitch, v(parity.data_ptr()), pitch, p * pitch, B, S,
                v(words.data_ptr()), v(located.data_ptr()), v(work.data_ptr()), work.numel(), 0, v(st.cuda_stream))
        assert rc == 0, rc

    def locate():
        call(L.shmr_ec_locate_batch_dev, data)

    def pair_clean():
        call(L.shmr_ec_locate_pair_batch_dev, data)

    def pair_damaged(skip):
        def run():
            call(L.shmr_ec_locate_pair_batch_dev, damaged)
        return run, skip

    legs = {"a_locate": (locate, 1), "a2_locate": (locate, 1), "b_pair_clean": (pair_clean, 1),
            "c_pair_damaged_skip": pair_damaged(1), "d_pair_damaged_all": pair_damaged(0)}

    def run(name, n):
        f, skip = legs[name]
        shmr_amd.set_tuning(pair_skip=skip)
        for _ in range(n):
            f()

    for n in legs:
        run(n, a.warmup)
    torch.cuda.synchronize()
    # the answers before anything is timed
    run("b_pair_clean", 1)
    torch.cuda.synchronize()
    assert not words.cpu().numpy().any() and (located.cpu().numpy() == -1).all()
    for n in ("c_pair_damaged_skip", "d_pair_damaged_all"):
        run(n, 1)
        torch.cuda.synchronize()
        loc = located.cpu().numpy().reshape(B, 2)
        assert (loc[hit] == [2, 7]).all() and (np.delete(loc, hit, 0) == -1).all(), loc
    times = {n: [] for n in legs}
    for _ in range(a.rounds):
        for n in legs:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            run(n, a.iters)
            e1.record(st)
            torch.cuda.synchronize()
            times[n].append(e0.elapsed_time(e1) / a.iters)
    shmr_amd.set_tuning(pair_skip=-2)
    med = {n: float(np.median(ts)) for n, ts in times.items()}
    lines = []
    for n, ts in times.items():
        rec = {"leg": n, "k": k, "p": p, "block_mib": MIB, "blocks": B, "shard_len": S, "pitch": pitch,
               "ms_per_call": round(med[n], 4), "ms_min": round(min(ts), 4), "ms_max": round(max(ts), 4),
               "ms_rounds": [round(t, 4) for t in ts], "over_a_locate": round(med[n] / med["a_locate"], 4),
               "rounds": a.rounds, "iters": a.iters, "flavour": _native.flavour(),
               "build_id": L.shmr_ec_build_id().decode()}
        if "damaged" in n:
            rec["damaged_blocks"] = len(hit)
            rec["ms_per_damaged_block"] = round((med[n] - med["b_pair_clean"]) / len(hit), 4)
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
