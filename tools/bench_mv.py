"""A/B of the two multi-vector score kernels in one process: option mv_tile = 0
(k_mv_simple, a lane per document) against mv_tile = 1 (k_mv_maxsim, the
LDS-staged wave-per-document kernel), alternating, each after a warm-up call of
its own.  Times are device events around the score and heap kernels of a call
(option timing, wv_mv_stats.last_kernel_ms) and the host's wall time of the
whole call (planner, uploads, kernels, download); results are compared bit for
bit in every row.

A row per (documents, tokens, d, query vectors, B, variant) gives ms per call
for each arm and the tiled kernel's share of the FMA floor: B * sum(tokens) *
T_q * d lane-operations over the non-packed f32 vector rate of the MI355X,
256 CUs x 64 lanes x 2.4 GHz = 39.3e12 lane-operations per second.

  python tools/bench_mv.py                              # every shape of the record
  python tools/bench_mv.py --tokens 32 --batches 1,16 --out /tmp/x.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

VALU_RATE = 256 * 64 * 2.4e9  # non-packed f32 lane-operations per second

ap = argparse.ArgumentParser()
ap.add_argument("--docs", type=int, default=40000)
ap.add_argument("--tokens", default="32,128", help="comma list of tokens per document")
ap.add_argument("--d", type=int, default=128)
ap.add_argument("--qv", type=int, default=32, help="query vectors per query")
ap.add_argument("--batches", default="1,16,256")
ap.add_argument("--variants", default="avx256,avx512")
ap.add_argument("--k", type=int, default=10)
ap.add_argument("--reps", type=int, default=3, help="timed calls per arm (after one warm-up each)")
ap.add_argument("--simple-max-s", type=float, default=20.0, help="skip the simple arm's repeats above this per call")
ap.add_argument("--arm", choices=["tile", "keys"], default="tile",
                help="tile: mv_tile 0 against 1; keys: mv_keys 0 against 1 (default --out profiles/mv_keys_ab.json)")
ap.add_argument("--nolist-docs", type=int, default=100000,
                help="--arm keys: documents of the corpus searched without allow lists (0: none)")
ap.add_argument("--out", default=None)
args = ap.parse_args()
if args.out is None:
    args.out = os.path.join(REPO, "profiles", "mv_keys_ab.json" if args.arm == "keys" else "mv_maxsim_ab.json")

import torch  # noqa: E402

if not torch.cuda.is_available():
    sys.exit("bench_mv.py needs a GPU")

import weaviate_amd as wv  # noqa: E402

rng = np.random.default_rng(1)
ids = np.arange(args.docs, dtype=np.uint64)
rows = []


def flush():
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "valu_rate_lane_ops_per_s": VALU_RATE,
                   "timing": "kernel_ms: device events around the score and heap kernels (and the key pass), best call; "
                             "call_ms: host wall time of the whole call, best call", "rows": rows}, f, indent=1)
        f.write("\n")


def fill(idx, docs, tokens):
    step = max(1, (64 << 20) // (tokens * args.d * 4))
    for i0 in range(0, docs, step):
        n = min(step, docs - i0)
        block = rng.random((n, tokens, args.d), dtype=np.float32) * 2 - 1
        idx.add_multi_batch(np.arange(i0, i0 + n, dtype=np.uint64), list(block))


def keys_arm():
    """mv_keys = 1 (k_mv_keys + k_mv_cut, the exact kernel on the survivors) against mv_keys = 0 (the exact
    kernel on every listed document), alternating; the listed corpora of the record, then the unlisted one."""
    corpora = [(args.docs, t, True) for t in (int(x) for x in args.tokens.split(","))]
    if args.nolist_docs:
        corpora.append((args.nolist_docs, int(args.tokens.split(",")[0]), False))
    for variant in args.variants.split(","):
        for docs, tokens, listed in corpora:
            idx = wv.MultiVectorIndex(distance="dot", dims=args.d, variant=variant)
            idx.set_option("timing", 1)
            idx.set_option("mv_keys_min", 0)
            fill(idx, docs, tokens)
            for B in (int(x) for x in args.batches.split(",")):
                queries = list(rng.random((B, args.qv, args.d), dtype=np.float32) * 2 - 1)
                allows = [np.arange(docs, dtype=np.uint64)] * B if listed else None
                best, out, st = {0: [1e30, 1e30], 1: [1e30, 1e30]}, {}, {}
                for rep in range(args.reps + 1):  # the first call of each arm is its warm-up
                    for arm in (0, 1):
                        idx.set_option("mv_keys", arm)
                        t0 = time.perf_counter()
                        out[arm] = idx.search_by_multi_vector_batch(queries, args.k, allows)
                        wall = (time.perf_counter() - t0) * 1e3
                        st[arm] = idx.stats()
                        if rep:
                            best[arm] = [min(best[arm][0], st[arm]["last_kernel_ms"] + st[arm]["last_key_ms"]),
                                         min(best[arm][1], wall)]
                same = all(np.array_equal(out[0][j].view(np.uint32) if j == 1 else out[0][j],
                                          out[1][j].view(np.uint32) if j == 1 else out[1][j]) for j in range(3))
                rows.append({"docs": docs, "tokens": tokens, "d": args.d, "query_vectors": args.qv, "B": B,
                             "variant": variant, "k": args.k, "allow_lists": listed,
                             "exact_kernel_ms": round(best[0][0], 3), "exact_call_ms": round(best[0][1], 3),
                             "keys_kernel_ms": round(best[1][0], 3), "keys_call_ms": round(best[1][1], 3),
                             "key_pass_ms": round(st[1]["last_key_ms"], 3),
                             "candidates_per_query": round(st[1]["last_candidates"] / B, 2),
                             "fallback_queries": st[1]["last_fallback_queries"], "route": st[1]["last_route"],
                             "same_results": bool(same)})
                print(json.dumps(rows[-1]), flush=True)
                flush()
            idx.close()


if args.arm == "keys":
    keys_arm()
    sys.exit(0)

for variant in args.variants.split(","):
    for tokens in (int(x) for x in args.tokens.split(",")):
        idx = wv.MultiVectorIndex(distance="dot", dims=args.d, variant=variant)
        idx.set_option("timing", 1)
        step = max(1, (64 << 20) // (tokens * args.d * 4))
        for i0 in range(0, args.docs, step):
            n = min(step, args.docs - i0)
            block = rng.random((n, tokens, args.d), dtype=np.float32) * 2 - 1
            idx.add_multi_batch(ids[i0:i0 + n], list(block))
        for B in (int(x) for x in args.batches.split(",")):
            queries = list(rng.random((B, args.qv, args.d), dtype=np.float32) * 2 - 1)
            allows = [ids] * B  # every query lists every document: the planner stores the list once
            best = {0: [1e30, 1e30], 1: [1e30, 1e30]}
            out = {}

            def call(tile):
                idx.set_option("mv_tile", tile)
                t0 = time.perf_counter()
                res = idx.search_by_multi_vector_batch(queries, args.k, allows)
                wall = (time.perf_counter() - t0) * 1e3
                return res, idx.stats()["last_kernel_ms"], wall

            warm = {}
            for tile in (0, 1):  # warm-up of each arm
                out[tile], km, wall = call(tile)
                warm[tile] = [km, wall]
            for _ in range(args.reps):
                for tile in (0, 1):
                    if tile == 0 and warm[0][1] > args.simple_max_s * 1e3:
                        best[0] = warm[0]  # a call of many seconds is timed once
                        continue
                    res, km, wall = call(tile)
                    best[tile] = [min(best[tile][0], km), min(best[tile][1], wall)]
            same = all(np.array_equal(out[0][j].view(np.uint32) if j == 1 else out[0][j],
                                      out[1][j].view(np.uint32) if j == 1 else out[1][j]) for j in range(3))
            floor_ms = B * args.docs * tokens * args.qv * args.d / VALU_RATE * 1e3
            rows.append({"docs": args.docs, "tokens": tokens, "d": args.d, "query_vectors": args.qv, "B": B,
                         "variant": variant, "k": args.k,
                         "simple_kernel_ms": round(best[0][0], 3), "tiled_kernel_ms": round(best[1][0], 3),
                         "simple_call_ms": round(best[0][1], 3), "tiled_call_ms": round(best[1][1], 3),
                         "fma_floor_ms": round(floor_ms, 3), "tiled_share_of_floor": round(floor_ms / best[1][0], 4),
                         "simple_share_of_floor": round(floor_ms / best[0][0], 4), "same_results": bool(same)})
            print(json.dumps(rows[-1]), flush=True)
            flush()
        idx.close()
