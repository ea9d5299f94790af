#!/usr/bin/env python3
"""Parity delta update (shmr_ec_update_batch_dev) against what a device Block
Cache had to do for the same writes before it existed: a device copy of the new
bytes into the data shards followed by encode_batch_dev of the touched blocks.
Interleaved rounds in one process, HIP events around each leg, on bench.py's
padded slots: RS(8,3) x 4 MiB x 512 resident blocks, separate data / parity
regions.  One update per block (the same shard and columns in every block):

  4k      4 KiB          64k     64 KiB
  shard   one whole shard (1/8 of the block's data)
  all     all k shards of every block (the update equals a fresh encode)

Legs per size: u_<size> the update, r_<size> copy + re-encode.  Both legs write
the same new bytes, so every leg leaves codewords behind (checked with
verify_batch_dev before anything is timed).  The update goes through the raw C
ABI call with a prebuilt update array, as a cache would hold it.

Algorithmic bytes: update (3 + 2p) * n per written byte range; re-encode 2n for
the copy plus (k + p) * S per block.  The last line derives, from the shard and
all legs of both sides (time linear in the written share between them), the
share of a block's data above which re-encoding wins.

    python tools/update_ab.py [--out profiles/r09/update_ab.jsonl]
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
SHARD, OFFSET = 3, 8192


def slot(S):
    pitch = (S + 4095) // 4096 * 4096
    return pitch + 4096 if pitch % 65536 == 0 else pitch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--iters", type=int, default=40, help="per round; the shard and all legs run a quarter of it")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default="", help="also append the JSON lines to this file")
    a = ap.parse_args()
    import shmr_amd
    from shmr_amd import _native

    assert torch.cuda.is_available(), "update_ab.py measures on the GPU"
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream()
    k, p, B = K, P, BLOCKS
    S = shmr_amd.calculate_shard_size(MIB << 20, k)
    pitch = slot(S)
    rs = shmr_amd.ReedSolomon(k, p)
    g = torch.Generator(device=dev)
    g.manual_seed(9)
    data = torch.randint(0, 256, (B, k, pitch), dtype=torch.uint8, device=dev, generator=g)
    parity = torch.zeros((B, p, pitch), dtype=torch.uint8, device=dev)
    rs.encode_batch_dev(data, parity, shard_len=S)              # the resident codewords
    src = torch.randint(0, 256, (B * k * S,), dtype=torch.uint8, device=dev, generator=g)
    words = torch.empty(B, dtype=torch.int32, device=dev)
    v = ctypes.c_void_p
    L = _native.lib()

    sizes = {"4k": (1, 4096), "64k": (1, 65536), "shard": (1, S), "all": (k, S)}
    legs, nbytes, iters = {}, {}, {}
    for name, (shards, n) in sizes.items():
        off = 0 if n == S else OFFSET
        first = 0 if shards == k else SHARD
        ups = np.array([(b, first + s, off, n, (b * shards + s) * n) for b in range(B) for s in range(shards)], dtype=np.int64)
        ua = rs._update_array(ups)

        def update(ua=ua):
            rc = L.shmr_ec_update_batch_dev(rs._h, v(data.data_ptr()), pitch, k * pitch, v(parity.data_ptr()), pitch,
                                            p * pitch, B, S, v(ua.ctypes.data), len(ua), v(src.data_ptr()), src.numel(),
                                            0, v(st.cuda_stream))
            assert rc == 0, rc

        new = src[:B * shards * n].view(B, shards, n)
        dst = data[:, first:first + shards, off:off + n]

        def reencode(new=new, dst=dst):
            dst.copy_(new)
            rs.encode_batch_dev(data, parity, shard_len=S)

        legs["u_" + name], legs["r_" + name] = update, reencode
        nbytes["u_" + name] = (3 + 2 * p) * n * shards * B
        nbytes["r_" + name] = 2 * n * shards * B + (k + p) * S * B
        iters["u_" + name] = iters["r_" + name] = a.iters if n < S else max(1, a.iters // 4)
    for n, f in legs.items():
        for _ in range(a.warmup):
            f()
        # every leg leaves codewords behind, before anything is timed
        rs.verify_batch_dev(data, parity, shard_len=S, out=words)
        torch.cuda.synchronize()
        assert not words.cpu().numpy().any(), n
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
    lines = []
    for n, ts in times.items():
        size = n[2:]
        lines.append(json.dumps({
            "leg": n, "k": k, "p": p, "block_mib": MIB, "blocks": B, "shard_len": S, "pitch": pitch,
            "updates": sizes[size][0] * B, "bytes_per_update": sizes[size][1],
            "ms_per_call": round(med[n], 4), "ms_min": round(min(ts), 4), "ms_max": round(max(ts), 4),
            "ms_rounds": [round(t, 4) for t in ts],
            "bytes": nbytes[n], "frac_hbm_peak": round(nbytes[n] / (med[n] / 1e3) / HBM_PEAK, 4),
            "reencode_over_update": round(med["r_" + size] / med["u_" + size], 3),
            "rounds": a.rounds, "iters": iters[n], "flavour": _native.flavour(),
            "build_id": L.shmr_ec_build_id().decode()}))
        print(lines[-1], flush=True)
    # time linear in the written share f of a block's data between f = 1/k and f = 1
    def line(side):
        t1, tk = med[side + "_shard"], med[side + "_all"]
        slope = (tk - t1) / (1 - 1 / k)
        return slope, t1 - slope / k
    (su, iu), (sr, ir) = line("u"), line("r")
    share = (ir - iu) / (su - sr) if su != sr else float("inf")
    lines.append(json.dumps({"leg": "breakeven", "update_ms_of_share": [round(su, 4), round(iu, 4)],
                             "reencode_ms_of_share": [round(sr, 4), round(ir, 4)],
                             "share_of_block_data_above_which_reencode_wins": round(share, 4),
                             "note": "ms = slope * share + intercept, from the shard (1/k) and all (1) legs"}))
    print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
