#!/usr/bin/env python3
"""Degraded update (shmr_ec_update_degraded_batch_dev) against what a device
Block Cache had to do for the same writes before the call existed:
reconstruct_batch_dev (data_only) of the whole batch, then update_batch_dev.
Interleaved rounds in one process, HIP events around each leg, on bench.py's
padded slots: RS(8,3) x 4 MiB x 512 resident blocks, block b has lost data shard
b mod k.  One update per block (the same columns in every block):

  4k      4 KiB       64k     64 KiB       256k    256 KiB       shard   the whole shard

Legs per size: u_<size> the degraded call into the lost shard, b_<size> rebuild
+ update of the same bytes; p_<size> the degraded call into the present shard
next to the lost one, q_<size> rebuild + update of those.  Two more pairs write
more of a block, to look for the size at which rebuilding first wins: u_two /
b_two the whole lost shard and the whole shard next to it (two rounds), u_all /
b_all all k data shards (k rounds).  Both legs of a pair leave the same bytes in
the present shards (compared before anything is timed).  Every call goes through
the raw C ABI with prebuilt arrays, as a cache would hold them.

Algorithmic bytes, n per update, S the shard length: the degraded call (k + 1 +
2p) * n into the lost shard and (3 + 2p) * n into a present one (all p parity
rows are present here); the baseline (k + 1) * S per block for the rebuild plus
(3 + 2p) * n.

    python tools/update_degraded_ab.py [--out profiles/r16/update_degraded_ab.jsonl]
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
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="", help="also append the JSON lines to this file")
    a = ap.parse_args()
    import shmr_amd
    from shmr_amd import _native

    assert torch.cuda.is_available(), "update_degraded_ab.py measures on the GPU"
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
    rows = torch.arange(B, device=dev)
    lost_t = torch.from_numpy(lost).to(dev)
    shards[rows, lost_t] = 0xEE                                        # the lost shards are gone
    start = shards.clone()
    src = torch.randint(0, 256, (B * k * S,), dtype=torch.uint8, device=dev, generator=g)
    v = ctypes.c_void_p
    L = _native.lib()
    pr = np.ascontiguousarray(present)
    there = torch.from_numpy(present.astype(bool)).to(dev)

    def degraded_leg(ups, buf=None):
        ua = rs._update_array(np.array(ups, dtype=np.int64))

        def f(buf=shards if buf is None else buf):
            rc = L.shmr_ec_update_degraded_batch_dev(rs._h, v(buf.data_ptr()), pitch, t * pitch,
                                                     pr.ctypes.data_as(_native._u8p), B, S, v(ua.ctypes.data), len(ua),
                                                     v(src.data_ptr()), src.numel(), 0, v(st.cuda_stream))
            assert rc == 0, rc
        return f

    def baseline_leg(ups, buf=None):
        ua = rs._update_array(np.array(ups, dtype=np.int64))

        def f(buf=shards if buf is None else buf):
            rc = L.shmr_ec_reconstruct_batch_dev(rs._h, v(buf.data_ptr()), pitch, t * pitch,
                                                 pr.ctypes.data_as(_native._u8p), B, S, 1, 0, v(st.cuda_stream))
            assert rc == 0, rc
            rc = L.shmr_ec_update_batch_dev(rs._h, v(buf.data_ptr()), pitch, t * pitch, v(buf.data_ptr() + k * pitch),
                                            pitch, t * pitch, B, S, v(ua.ctypes.data), len(ua), v(src.data_ptr()),
                                            src.numel(), 0, v(st.cuda_stream))
            assert rc == 0, rc
        return f

    sizes = {"4k": 4096, "64k": 65536, "256k": 262144, "shard": S}
    lists, nbytes, written = {}, {}, {}
    for name, n in sizes.items():
        off = 0 if n == S else OFFSET
        lists["u_" + name] = lists["b_" + name] = [(b, int(lost[b]), off, n, b * n) for b in range(B)]
        lists["p_" + name] = lists["q_" + name] = [(b, int(near[b]), off, n, b * n) for b in range(B)]
        nbytes["u_" + name] = (k + 1 + 2 * p) * n * B
        nbytes["p_" + name] = (3 + 2 * p) * n * B
        nbytes["b_" + name] = nbytes["q_" + name] = ((k + 1) * S + (3 + 2 * p) * n) * B
        for leg in "ubpq":
            written[leg + "_" + name] = n
    lists["u_two"] = lists["b_two"] = [(b, int(s), 0, S, (2 * b + i) * S) for b in range(B)
                                       for i, s in enumerate((lost[b], near[b]))]
    lists["u_all"] = lists["b_all"] = [(b, s, 0, S, (k * b + s) * S) for b in range(B) for s in range(k)]
    nbytes["u_two"] = ((k + 1 + 2 * p) + (3 + 2 * p)) * S * B
    nbytes["b_two"] = ((k + 1) + 2 * (3 + 2 * p)) * S * B
    nbytes["u_all"] = ((k + 1 + 2 * p) + (k - 1) * (3 + 2 * p)) * S * B
    nbytes["b_all"] = ((k + 1) + k * (3 + 2 * p)) * S * B
    written.update(u_two=2 * S, b_two=2 * S, u_all=k * S, b_all=k * S)
    pair = {"u": "b", "b": "u", "p": "q", "q": "p"}
    legs = {n: (degraded_leg if n[0] in "up" else baseline_leg)(ups) for n, ups in lists.items()}
    iters = {n: a.iters if (written[n] < S and n[0] in "up") else max(1, a.iters // 4) for n in legs}
    # both legs of a pair leave the same bytes in the present shards, before anything is timed
    twin = torch.empty_like(shards)
    for n, ups in lists.items():
        if n[0] not in "up":
            continue
        shards.copy_(start)
        twin.copy_(start)
        legs[n]()
        baseline_leg(ups, twin)()
        torch.cuda.synchronize()
        assert torch.equal(shards[:, :, :S][there], twin[:, :, :S][there]), n
        assert bool((shards[rows, lost_t] == 0xEE).all()), n + ": a lost slot was written"
    del twin
    shards.copy_(start)
    for f in legs.values():
        for _ in range(a.warmup):
            f()
    torch.cuda.synchronize()
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
        leg, size = n[0], n[2:]
        ours, base = (n, pair[leg] + "_" + size) if leg in "up" else (pair[leg] + "_" + size, n)
        lines.append(json.dumps({
            "leg": n, "k": k, "p": p, "block_mib": MIB, "blocks": B, "shard_len": S, "pitch": pitch,
            "updates": len(lists[n]), "bytes_written_per_block": written[n],
            "ms_per_call": round(med[n], 4), "ms_min": round(min(ts), 4), "ms_max": round(max(ts), 4),
            "ms_rounds": [round(x, 4) for x in ts],
            "bytes": nbytes[n], "frac_hbm_peak": round(nbytes[n] / (med[n] / 1e3) / HBM_PEAK, 4),
            "baseline_over_degraded": round(med[base] / med[ours], 3),
            "rounds": a.rounds, "iters": iters[n], "flavour": _native.flavour(),
            "build_id": L.shmr_ec_build_id().decode()}))
        print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
