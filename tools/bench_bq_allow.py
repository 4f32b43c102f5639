#!/usr/bin/env python3
"""Filtered serving on a compressed flat index: per-query allow lists in one
shared launch against the grouped path (one complete search per distinct
list).  --compression bq: option pqa_bq; rq8 / rq1: option
pqa_rq, DESIGN §3.9e.

Corpus: n x 768 cosine rows from wv_gen_device, k = 10, rescore_limit -1 and
100.  Batches of B queries, each with its own random allow list at a density
of 50 %, 10 % or 1 %, plus one mix (a quarter of the queries unfiltered, the
rest at 10 %).  The two arms alternate in one process after a warm-up call of
each; the clock is the wall clock around the synchronous host call
(wv_index_search_by_vector_batch_multi_allow on prebuilt arrays), each arm gets
at least --seconds of timed work, and the two arms' results are compared bit
for bit in every cell.  For rq each cell also records how many of the shared
arm's queries were replayed (the rest were proven from their candidates).

    python tools/bench_bq_allow.py --out profiles/bq_pqa_ab.json
    python tools/bench_bq_allow.py --compression rq8 --out profiles/rq_pqa_ab.json
    python tools/bench_bq_allow.py --compression rq1 --out profiles/rq_pqa_ab.json --append

The default grid (24 cells per compression) takes about ten minutes: both arms
run until the faster one has its --seconds.  --append adds this process's
cells to the record already at --out (one process per compression keeps each
run inside a ten-minute slot); the record's "runs" lists the processes.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

SEED_CORPUS, SEED_QUERY = 20240601, 20240602


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--dims", type=int, default=768)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--batches", type=int, nargs="+", default=[16, 64, 256])
    ap.add_argument("--rescore", type=int, nargs="+", default=[-1, 100])
    ap.add_argument("--seconds", type=float, default=1.0, help="timed work per arm and cell, at least")
    ap.add_argument("--compression", nargs="+", choices=["bq", "rq8", "rq1"], default=["bq"])
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "bq_pqa_ab.json"))
    ap.add_argument("--append", action="store_true", help="add the cells to the record already at --out")
    args = ap.parse_args()

    import torch
    import weaviate_amd as wv
    from weaviate_amd import _lib
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    n, d, k = args.n, args.dims, args.k

    bmax = max(args.batches)
    qd = torch.empty((bmax, d), dtype=torch.float32, device=dev)
    _lib.check(lib.wv_gen_device(0, 0, SEED_QUERY, 0, bmax, d, qd.data_ptr(), None))
    torch.cuda.synchronize()
    queries = np.ascontiguousarray(qd.cpu().numpy())
    del qd

    cells = []
    for comp in args.compression:
        cells += run_compression(args, comp, wv, _lib, lib, torch, queries)
    names = " / ".join(c.upper() if c == "bq" else c[:2] + "-" + c[2:] for c in args.compression)
    opts = " / ".join(sorted({OPTION[c] for c in args.compression}))
    rec = {"tool": "tools/bench_bq_allow.py", "device": torch.cuda.get_device_name(0),
           "corpus": f"{n} x {d} cosine {names} (wv_gen_device kind 0), k = {k}",
           "clock": "wall clock around the synchronous host call, median per call; arms alternate, "
                    f">= {args.seconds} s of timed work per arm and cell",
           "arms": {"grouped": f"{opts} = 0: one search per distinct list",
                    "shared": f"{opts} = 1: union minima once, per-query replays"},
           "runs": [list(args.compression)],
           "cells": cells, "all_bit_equal": all(c["bit_equal"] for c in cells)}
    if args.append and os.path.exists(args.out):
        with open(args.out) as f:
            rec = merge_records(json.load(f), rec)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    return 0 if rec["all_bit_equal"] else 1


OPTION = {"bq": "pqa_bq", "rq8": "pqa_rq", "rq1": "pqa_rq"}


def merge_records(old, new):
    """--append: the earlier record with this process's cells after its own"""
    rec = dict(old)
    rec["corpus"] = old["corpus"] if old["corpus"] == new["corpus"] else [old["corpus"], new["corpus"]]
    rec["runs"] = old.get("runs", []) + new["runs"]
    rec["cells"] = old["cells"] + new["cells"]
    rec["all_bit_equal"] = all(c["bit_equal"] for c in rec["cells"])
    return rec


def run_compression(args, comp, wv, _lib, lib, torch, queries):
    """the grid of cells on one index of compression `comp`"""
    fp, up, ip = C.POINTER(C.c_float), C.POINTER(C.c_uint64), C.POINTER(C.c_int32)
    n, d, k = args.n, args.dims, args.k
    opt = OPTION[comp]
    kw = {"bq": True} if comp == "bq" else {"rq": {"bits": int(comp[2:])}}
    index = wv.FlatIndex(distance="cosine", dims=d, device=0, variant="avx256", **kw)
    index.reserve(n)
    stage = torch.empty((n, d), dtype=torch.float32, device=torch.device("cuda", 0))
    _lib.check(lib.wv_gen_device(0, 0, SEED_CORPUS, 0, n, d, stage.data_ptr(), None))
    _lib.check(lib.wv_index_add_range_device(index._h, 0, stage.data_ptr(), n, d))
    del stage

    def call(B, aids, off, modes, out):
        ids, dists, counts = out
        _lib.check(lib.wv_index_search_by_vector_batch_multi_allow(
            index._h, queries.ctypes.data_as(fp), B, d, k, aids.ctypes.data_as(up), off.ctypes.data_as(C.c_void_p),
            modes.ctypes.data_as(ip), ids.ctypes.data_as(up), dists.ctypes.data_as(fp), counts.ctypes.data_as(ip)))

    rng = np.random.default_rng(7)
    cells = []
    for R in args.rescore:
        index.set_option("rescore_limit", R)
        for B in args.batches:
            for name, dens, unf in (("50%", 0.5, 0.0), ("10%", 0.1, 0.0), ("1%", 0.01, 0.0), ("mix", 0.1, 0.25)):
                modes = np.ones(B, dtype=np.int32)
                modes[: int(B * unf)] = 0
                parts = [np.flatnonzero(rng.random(n) < dens).astype(np.uint64) if modes[q] else np.zeros(0, np.uint64)
                         for q in range(B)]
                off = np.zeros(B + 1, dtype=np.int64)
                off[1:] = np.cumsum([p.size for p in parts])
                aids = np.ascontiguousarray(np.concatenate(parts + [np.zeros(1, np.uint64)]))
                del parts
                outs = [(np.zeros((B, k), np.uint64), np.zeros((B, k), np.float32), np.zeros(B, np.int32))
                        for _ in range(2)]
                for arm in (0, 1):  # warm-up of each arm
                    index.set_option(opt, arm)
                    call(B, aids, off, modes, outs[arm])
                times = [[], []]
                nb = [0, 0]
                nrep = [0, 0]
                while min(sum(times[0]), sum(times[1])) < args.seconds or len(times[0]) < 3:
                    for arm in (0, 1):
                        index.set_option(opt, arm)
                        st0 = index.stats()
                        t0 = time.perf_counter()
                        call(B, aids, off, modes, outs[arm])
                        times[arm].append(time.perf_counter() - t0)
                        st1 = index.stats()
                        nb[arm] = st1["batches"] - st0["batches"]
                        nrep[arm] = st1["replayed_queries"] - st0["replayed_queries"]
                equal = all(np.array_equal(outs[0][j].view(np.uint32 if j == 1 else outs[0][j].dtype),
                                           outs[1][j].view(np.uint32 if j == 1 else outs[1][j].dtype)) for j in range(3))
                cell = {"compression": comp, "rescore_limit": R, "B": B, "lists": name,
                        "grouped_ms": round(1e3 * float(np.median(times[0])), 3),
                        "shared_ms": round(1e3 * float(np.median(times[1])), 3),
                        "grouped_calls": len(times[0]), "shared_calls": len(times[1]),
                        "grouped_batches": int(nb[0]), "shared_batches": int(nb[1]), "bit_equal": bool(equal)}
                cell["speedup"] = round(cell["grouped_ms"] / cell["shared_ms"], 2)
                if comp != "bq":  # search_rq: proven from the candidates, or replayed
                    cell["shared_replayed"] = int(nrep[1])
                    cell["shared_proven"] = int(B - nrep[1])
                    cell["grouped_replayed"] = int(nrep[0])
                print(json.dumps(cell), flush=True)
                cells.append(cell)
                del aids
    index.set_option(opt, 1)
    index.close()
    return cells


if __name__ == "__main__":
    sys.exit(main())
