#!/usr/bin/env python3
"""Ranged reads (shmr_ec_read_batch_dev) against what a device Block Cache had
to do for the same reads before the call existed: reconstruct_batch_dev_out
(data_only) of the whole batch into a compact output, followed by a device copy
of the requested ranges out of it.  Interleaved rounds in one process, HIP
events around each leg, on bench.py's padded slots: RS(8,3) x 4 MiB x 512
resident blocks, block b has lost data shard b mod k.  One request per block
(the same columns in every block) into the lost shard:

  4k      4 KiB          64k     64 KiB          shard   the whole shard

Legs per size: r_<size> the read call, b_<size> rebuild + copy; and a copy-only
pair, requests into the present shard next to the lost one: c_<size> the read
call, g_<size> a torch gather of the same ranges.  Both legs of a pair fill the
same destination bytes (compared before anything is timed).  The read goes
through the raw C ABI call with a prebuilt request array, as a cache would hold
it.

Algorithmic bytes: rebuild leg of the read (k + 1) * n per request, copy leg
2 * n; the baseline (k + 1) * S per block plus 2 * n for the copy.  The traffic
model predicts a ratio near S / n at small ranges and near 1 at a whole shard.

    python tools/read_ab.py [--out profiles/r13/read_ab.jsonl]
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
OFFSET = 8192


def slot(S):
    pitch = (S + 4095) // 4096 * 4096
    return pitch + 4096 if pitch % 65536 == 0 else pitch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--iters", type=int, default=40, help="per round; the baseline and whole-shard legs run a quarter of it")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default="", help="also append the JSON lines to this file")
    a = ap.parse_args()
    import shmr_amd
    from shmr_amd import _native

    assert torch.cuda.is_available(), "read_ab.py measures on the GPU"
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream()
    k, p, B = K, P, BLOCKS
    t = k + p
    S = shmr_amd.calculate_shard_size(MIB << 20, k)
    pitch = slot(S)
    rs = shmr_amd.ReedSolomon(k, p)
    g = torch.Generator(device=dev)
    g.manual_seed(10)
    shards = torch.randint(0, 256, (B, t, pitch), dtype=torch.uint8, device=dev, generator=g)
    rs.encode_batch_dev(shards[:, :k], shards[:, k:], shard_len=S)     # the resident codewords
    lost = np.arange(B) % k
    near = (lost + 1) % k
    present = np.ones((B, t), dtype=np.uint8)
    present[np.arange(B), lost] = 0
    truth = shards[torch.arange(B, device=dev), torch.from_numpy(lost).to(dev)].clone()
    shards[torch.arange(B, device=dev), torch.from_numpy(lost).to(dev)] = 0xEE     # the lost shards are gone
    rebuilt = torch.zeros((B, 1, pitch), dtype=torch.uint8, device=dev)
    dst = torch.zeros(B * S, dtype=torch.uint8, device=dev)
    rows = torch.arange(B, device=dev)
    near_t = torch.from_numpy(near).to(dev)
    v = ctypes.c_void_p
    L = _native.lib()
    pr = np.ascontiguousarray(present)

    sizes = {"4k": 4096, "64k": 65536, "shard": S}
    legs, nbytes, iters, check = {}, {}, {}, {}
    for name, n in sizes.items():
        off = 0 if n == S else OFFSET

        def read_leg(which, n=n, off=off):
            ra = rs._read_array(np.array([(b, which[b], off, n, b * n) for b in range(B)], dtype=np.int64))

            def f(ra=ra):
                rc = L.shmr_ec_read_batch_dev(rs._h, v(shards.data_ptr()), pitch, t * pitch, pr.ctypes.data_as(_native._u8p),
                                              B, S, v(ra.ctypes.data), len(ra), v(dst.data_ptr()), dst.numel(), 0,
                                              v(st.cuda_stream))
                assert rc == 0, rc
            return f

        def baseline(n=n, off=off):
            rs.reconstruct_batch_dev_out(shards, present, rebuilt, shard_len=S, data_only=True)
            dst[:B * n].view(B, n).copy_(rebuilt[:, 0, off:off + n])

        def gather(n=n, off=off):
            dst[:B * n].view(B, n).copy_(shards[rows, near_t, off:off + n])

        legs["r_" + name], legs["b_" + name] = read_leg(lost), baseline
        legs["c_" + name], legs["g_" + name] = read_leg(near), gather
        nbytes["r_" + name] = (k + 1) * n * B
        nbytes["b_" + name] = (k + 1) * S * B + 2 * n * B
        nbytes["c_" + name] = nbytes["g_" + name] = 2 * n * B
        for leg in "rbcg":
            iters[leg + "_" + name] = a.iters if (n < S and leg != "b") else max(1, a.iters // 4)
        check[name] = (n, off)
    # both legs of a pair fill the same destination bytes, before anything is timed
    for name, (n, off) in check.items():
        want = {"r": truth[:, off:off + n], "b": truth[:, off:off + n],
                "c": shards[rows, near_t, off:off + n], "g": shards[rows, near_t, off:off + n]}
        for leg in "rbcg":
            dst.zero_()
            for _ in range(a.warmup):
                legs[leg + "_" + name]()
            torch.cuda.synchronize()
            assert torch.equal(dst[:B * n].view(B, n), want[leg]), leg + "_" + name
    times = {n: [] for n in legs}
    for _ in range(a.rounds):
        for n, f in legs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            for _ in range(iters[n]):
                f()
            e1.record(st)
            torch.cuda.synchronize()
            times[n].append(e0.elapsed_time(e1) / iters[n])
    med = {n: float(np.median(ts)) for n, ts in times.items()}
    pair = {"r": "b", "b": "r", "c": "g", "g": "c"}
    lines = []
    for n, ts in times.items():
        leg, size = n[0], n[2:]
        ours, base = (n, pair[leg] + "_" + size) if leg in "rc" else (pair[leg] + "_" + size, n)
        lines.append(json.dumps({
            "leg": n, "k": k, "p": p, "block_mib": MIB, "blocks": B, "shard_len": S, "pitch": pitch,
            "requests": B, "bytes_per_request": sizes[size],
            "ms_per_call": round(med[n], 4), "ms_min": round(min(ts), 4), "ms_max": round(max(ts), 4),
            "ms_rounds": [round(x, 4) for x in ts],
            "bytes": nbytes[n], "frac_hbm_peak": round(nbytes[n] / (med[n] / 1e3) / HBM_PEAK, 4),
            "baseline_over_read": round(med[base] / med[ours], 3),
            "rounds": a.rounds, "iters": iters[n], "flavour": _native.flavour(),
            "build_id": L.shmr_ec_build_id().decode()}))
        print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
