#!/usr/bin/env python3
"""Generates the committed golden fixtures under tests/golden/.

Two kinds of data, kept apart on purpose:

* kat.json "published" -- known-answer values of the crate the reference calls
  (reed-solomon-erasure 6.0.0, itself a port of Backblaze JavaReedSolomon):
  galois multiply/exp/slice-multiply KATs, the matrix multiply/invert tests
  and the RS(5,5) encode vector.  These pin the
  oracle to the upstream algorithm; they are data, not code.
* everything else -- produced by this repo's CPU oracle (oracle/rs_oracle.py)
  from seeded inputs: parity rows of the BASELINE configs, small blocks in full
  bytes, benchmark-sized blocks as SHA-256 per shard, shmr glue cases
  (calculate_shard_size f32 edges, sync_data partial buffers, load_block
  quirks).  These are the build's own pins (regression vectors).

Run:  python tests/golden/make_golden.py

* tuning_table.json -- what the two native libraries answer to the tuning
  calls (every knob, key form and value) and their describe strings: recorded
  from a build of the commit whose behaviour is to be kept, replayed by
  tests/test_abi.py.

Run:  python tests/golden/make_golden.py tuning_table <directory of the two libraries>
"""
from __future__ import annotations

import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from oracle import rs_oracle as O  # noqa: E402

SEED = O.BENCH_SEED


def sha(a: np.ndarray) -> str:
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


_SLICE_IN = [0, 1, 2, 3, 4, 5, 6, 10, 50, 100, 150, 174, 201, 255, 99, 32, 67, 85]


def published_kats():
    return {
        "source": "reed-solomon-erasure 6.0.0 galois_8 tests / Backblaze JavaReedSolomon (published KATs)",
        "gal_mul": [[3, 4, 12], [7, 7, 21], [23, 45, 41]],
        "gal_exp": [[2, 2, 4], [5, 20, 235], [13, 7, 43]],
        "encode": [{"data_shards": 5, "parity_shards": 5,
                    "data": [[0, 1], [4, 5], [2, 3], [6, 7], [8, 9]],
                    "parity": [[12, 13], [10, 11], [14, 15], [90, 91], [94, 95]]}],
        # galois slice multiply (upstream test_slice_mul / galMulSlice): [c, in, expected]
        "mul_slice": [
            [25, _SLICE_IN, [0x00, 0x19, 0x32, 0x2b, 0x64, 0x7d, 0x56, 0xfa, 0xb8, 0x6d, 0xc7, 0x85, 0xc3,
                             0x1f, 0x22, 0x07, 0x25, 0xfe]],
            [177, _SLICE_IN, [0x00, 0xb1, 0x7f, 0xce, 0xfe, 0x4f, 0x81, 0x9e, 0x03, 0x06, 0xe8, 0x75, 0xbd,
                              0x40, 0x36, 0xa3, 0x95, 0xcb]],
        ],
        # matrix tests (upstream MatrixTest / matrix.rs tests): [a, b, a*b] and [m, inv(m)]
        "mat_mul": [[[[1, 2], [3, 4]], [[5, 6], [7, 8]], [[11, 22], [19, 42]]]],
        "mat_invert": [
            [[[56, 23, 98], [3, 100, 200], [45, 201, 123]], [[175, 133, 33], [130, 13, 245], [112, 35, 126]]],
            [[[1, 0, 0, 0, 0], [0, 1, 0, 0, 0], [0, 0, 0, 1, 0], [0, 0, 0, 0, 1], [7, 7, 6, 6, 1]],
             [[1, 0, 0, 0, 0], [0, 1, 0, 0, 0], [123, 123, 1, 122, 122], [0, 0, 1, 0, 0], [0, 0, 0, 1, 0]]],
        ],
    }


def build_pins():
    pins = {"parity_rows": {}, "shard_size": [], "tables": {}}
    for k, p in [(4, 2), (8, 3), (10, 4), (5, 5), (1, 1), (2, 1), (17, 3), (200, 56)]:
        pins["parity_rows"][f"{k},{p}"] = O.ReedSolomon(k, p).parity_rows().tolist()
    for length, k in [(1 << 20, 4), (4 << 20, 8), (16 << 20, 10), (7000, 4), (16777217, 8), (16777221, 10),
                      (16777216, 3), (1, 7), (0, 3), (33554433, 16), (100, 3)]:
        pins["shard_size"].append([length, k, O.calculate_shard_size(length, k)])
    pins["tables"] = {"log_sha256": sha(O.LOG_TABLE), "exp_sha256": sha(O.EXP_TABLE),
                      "mul_sha256": sha(O.MUL_TABLE)}
    return pins


def small_vectors():
    """Full-byte vectors, small enough to commit as .npz."""
    out = {}
    cases = [(4, 2, 1024), (8, 3, 777), (10, 4, 1000), (3, 3, 17), (1, 1, 5), (6, 2, 4096 + 3)]
    for ci, (k, p, L) in enumerate(cases):
        rng = np.random.default_rng([SEED, 1000 + ci])
        data = rng.integers(0, 256, (k, L), dtype=np.uint8)
        sh = [d.copy() for d in data] + [np.zeros(L, np.uint8) for _ in range(p)]
        O.ReedSolomon(k, p).encode(sh)
        out[f"enc_{k}_{p}_{L}_data"] = data
        out[f"enc_{k}_{p}_{L}_parity"] = np.stack(sh[k:])
    # reconstruct vectors: inconsistent (random) shards exercise the crate's
    # "first k present + re-encode parity" rule
    k, p, L = 4, 3, 64
    rng = np.random.default_rng([SEED, 2000])
    shards = rng.integers(0, 256, (k + p, L), dtype=np.uint8)
    out["rec_4_3_shards"] = shards
    pats = [[0], [6], [0, 4], [1, 2, 3], [3, 5, 6], [0, 1, 2]]
    results = []
    for miss in pats:
        got = [None if i in miss else shards[i].copy() for i in range(k + p)]
        O.ReedSolomon(k, p).reconstruct(got)
        results.append(np.stack(got))
    out["rec_4_3_missing"] = np.array([m + [-1] * (3 - len(m)) for m in pats], dtype=np.int16)
    out["rec_4_3_result"] = np.stack(results)
    return out


def large_vectors():
    """Benchmark-sized blocks as SHA-256 per shard (inputs regenerated from seed)."""
    out = []
    for k, p, size, idx in [(4, 2, 1 << 20, 0), (8, 3, 4 << 20, 0), (8, 3, 4 << 20, 1), (10, 4, 16 << 20, 0)]:
        S = O.calculate_shard_size(size, k)
        buf = O.seeded_block(SEED, idx, size)
        shards = O.sync_data_erasure(buf.tobytes(), size, k, p)
        out.append({"k": k, "p": p, "block_bytes": size, "seed": [SEED, idx], "shard_bytes": S,
                    "generator": "numpy.random.default_rng([seed, idx]).integers(0, 256, block_bytes, uint8)",
                    "shard_sha256": [sha(s) for s in shards]})
    # edge blocks: all-0x00, all-0xFF, partial buffer 700,001 B
    for name, buf in [("zeros", np.zeros(1 << 20, np.uint8)), ("ones", np.full(1 << 20, 0xFF, np.uint8)),
                      ("partial_700001", O.seeded_block(SEED, 7, 700001))]:
        shards = O.sync_data_erasure(buf.tobytes(), 1 << 20, 4, 2)
        out.append({"k": 4, "p": 2, "block_bytes": 1 << 20, "case": name, "buffer_len": int(buf.size),
                    "seed": [SEED, 7] if name.startswith("partial") else None,
                    "shard_sha256": [sha(s) for s in shards]})
    return out


def f32_hazard_release():
    """block.rs:421's u8 wrap in the reference's release build: a full
    16,777,217 B Erasure(1,8,3) buffer (9 chunks of S = 2,097,152) encodes
    into k+p shards with chunk 8 overwritten by parity row 0
    (oracle sync_data_erasure, mode="release")."""
    size, k, p = 16777217, 8, 3
    buf = O.seeded_block(SEED, 9, size)
    shards = O.sync_data_erasure(buf.tobytes(), size, k, p, mode="release")
    loaded = O.load_block_erasure([s.tobytes() for s in shards], size, k, p)
    return {"k": k, "p": p, "block_bytes": size, "buffer_len": size, "seed": [SEED, 9],
            "shard_bytes": O.calculate_shard_size(size, k),
            "generator": "numpy.random.default_rng([seed, idx]).integers(0, 256, block_bytes, uint8)",
            "shard_sha256": [sha(s) for s in shards], "load_block_sha256": sha(loaded),
            "lost_byte_offset": k * O.calculate_shard_size(size, k), "lost_byte": int(buf[-1]),
            "loaded_last_byte": int(loaded[-1])}


def glue_cases():
    """load_block quirks (src/vfs/block.rs:529-579)."""
    k, p, size = 4, 2, 4096
    buf = O.seeded_block(SEED, 42, size)
    shards = O.sync_data_erasure(buf.tobytes(), size, k, p)
    cases = {}
    # a read error on data shard 1 -> None -> reconstructed
    s1 = [bytes(x) for x in shards]
    s1[1] = None
    cases["read_error_data1"] = sha(O.load_block_erasure(s1, size, k, p))
    # a truncated shard is zero-padded and stays "present" -> reconstruct is a
    # no-op when every shard is Some, so the zero padding survives
    s2 = [bytes(x) for x in shards]
    s2[2] = s2[2][:100]
    cases["truncated_data2"] = sha(O.load_block_erasure(s2, size, k, p))
    cases["intact"] = sha(O.load_block_erasure([bytes(x) for x in shards], size, k, p))
    cases["original"] = sha(buf)
    return cases


TUNING_VALUES = [-3, -2, -1, 0, 1, 2, 3, 4, 5, 6, 7, 9, 32, 33, 64, 128, 256, 512, 65536, 65537, 10000001]
KERNEL_FLAGS = ["nt_load", "nt_store", "occ8", "diag", "early", "spre", "fuse_tail", "glds", "serial", "sc1_store",
                "realign", "peel", "wave_run", "st_align", "xcd", "pair"]
# kernel knob -> the non-default values its describe strings are recorded under
KERNEL_KNOBS = {"chunks": [2], "grid": [0], "threads": [128], "depth": [3], "wgs_per_cu": [4], "occ": [6],
                **{name: [0, 1] for name in KERNEL_FLAGS}}
PROCESS_KNOBS = ["bounce_kib", "mirror_zc", "ptrs_segs", "ptrs_grid", "ptrs_direct", "sync_spin_us", "uvec",
                 "pattern_launches", "lattice_list", "slots_list", "alias_devices"]
SUBMIT_KNOBS = ["coalesce", "coalesce_depth", "coalesce_target", "coalesce_us", "coalesce_max", "coalesce_spin_us",
                "coalesce_watch_us", "coalesce_mark", "coalesce_lead_us", "coalesce_idle_us"]
TUNING_NAMES = list(KERNEL_KNOBS) + PROCESS_KNOBS + SUBMIT_KNOBS + ["no_such_knob", "encode.coalesce",
                                                                    "encode.bounce_kib"]
TUNING_RESET = {"occ8": 0, "diag": 0, "threads": 256, "grid": -1}   # every other knob resets with -2


def tuning_record(L):
    """What one library (a ctypes handle with shmr_amd._native's signatures)
    answers to the tuning calls; no device is touched.  "keys": per name one
    row for each form of the key (bare, with "encode.", with "decode."): per
    TUNING_VALUES entry the status of shmr_ec_set_tuning, then shmr_ec_get_tuning
    of the three forms, the knob reset after each entry.  "describe": shmr_ec_describe_variant
    for decode 0..4 x data_shards {4, 8, 9, 10} x rows 1..5 at default tuning
    and, in the tools build, under each kernel knob set alone."""
    import ctypes

    def reset(name):
        L.shmr_ec_set_tuning(name.encode(), TUNING_RESET.get(name, -2))

    def describe():
        buf, out = ctypes.create_string_buffer(512), []
        for decode in range(5):
            for k in (4, 8, 9, 10):
                for rows in range(1, 6):
                    rc = L.shmr_ec_describe_variant(decode, k, rows, buf, len(buf))
                    out.append(buf.value.decode() if rc == 0 else f"status {rc}")
        return out

    keys = {}
    for name in TUNING_NAMES:
        forms = [f.encode() for f in (name, "encode." + name, "decode." + name)]
        keys[name] = []
        for key in forms:
            row = []
            for v in TUNING_VALUES:
                row.append(L.shmr_ec_set_tuning(key, v))
                row += [L.shmr_ec_get_tuning(f) for f in forms]
                reset(name)
            keys[name].append(row)
    desc = {"default": describe()}
    if L.shmr_ec_is_tools_build():
        for name, values in KERNEL_KNOBS.items():
            for cls in ("encode.", "decode."):
                for v in values:
                    assert L.shmr_ec_set_tuning((cls + name).encode(), v) == 0, (cls, name, v)
                    desc[f"{cls}{name}={v}"] = describe()
                    reset(name)
        assert describe() == desc["default"]
    return {"keys": keys, "describe": desc}


def _interned(table, item):
    """Index of `item` in `table` (appended when new): rows and strings repeat."""
    if item not in table:
        table.append(item)
    return table.index(item)


def tuning_table(lib_dir):
    """tests/golden/tuning_table.json from the two libraries in `lib_dir`
    (built from the commit whose behaviour is to be kept)."""
    import ctypes
    from shmr_amd import _native
    out = {"values": TUNING_VALUES, "rows": [], "strings": []}
    for flavour, so in (("product", "libshmr_ec.so"), ("tools", "libshmr_ec_tools.so")):
        L = ctypes.CDLL(os.path.join(lib_dir, so))
        for name, res, args in _native.SIGNATURES:
            getattr(L, name).restype, getattr(L, name).argtypes = res, args
        rec = tuning_record(L)
        assert tuning_record(L) == rec, "not reproducible within one process"
        out[flavour + ".keys"] = {k: [_interned(out["rows"], r) for r in rows]
                                   for k, rows in rec["keys"].items()}
        out[flavour + ".describe"] = {c: [_interned(out["strings"], s) for s in d]
                                      for c, d in rec["describe"].items()}
    return out


def tuning_unpacked(table, flavour):
    """The tuning_record() a packed tuning_table() holds for one flavour."""
    return {"keys": {k: [table["rows"][i] for i in rows] for k, rows in table[flavour + ".keys"].items()},
            "describe": {c: [table["strings"][i] for i in d] for c, d in table[flavour + ".describe"].items()}}


def write_tuning_table(lib_dir):
    """One table entry per line (compact, and a change shows as changed lines)."""
    def dumps(x):
        return json.dumps(x, separators=(",", ":"))
    table, parts = tuning_table(lib_dir), []
    for name, value in table.items():
        if isinstance(value, dict):
            body = ",\n".join(f"{dumps(k)}:{dumps(v)}" for k, v in value.items())
            parts.append(f"{dumps(name)}:{{\n{body}\n}}")
        elif name == "values":
            parts.append(f"{dumps(name)}:{dumps(value)}")
        else:
            parts.append(f"{dumps(name)}:[\n" + ",\n".join(dumps(v) for v in value) + "\n]")
    path = os.path.join(HERE, "tuning_table.json")
    with open(path, "w") as f:
        f.write("{\n" + ",\n".join(parts) + "\n}\n")
    print("wrote", path)


def main():
    if len(sys.argv) == 3 and sys.argv[1] == "tuning_table":   # make_golden.py tuning_table <dir of the libraries>
        return write_tuning_table(sys.argv[2])
    kat = {"published": published_kats(), "build_pins": build_pins(), "large": large_vectors(),
           "load_block": glue_cases(), "f32_hazard_release": f32_hazard_release()}
    with open(os.path.join(HERE, "kat.json"), "w") as f:
        json.dump(kat, f, indent=1)
    np.savez_compressed(os.path.join(HERE, "small_vectors.npz"), **small_vectors())
    print("wrote", os.path.join(HERE, "kat.json"), "and small_vectors.npz")


if __name__ == "__main__":
    main()
