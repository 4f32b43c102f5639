"""A/B of hnsw's flat search with one allow list per query, in one process.

Corpus from wv_gen_device (1 M rows, d = 768), k = 10, 64 queries, every query
with its own random ascending list of --lens ids (the reference takes this
branch below flatSearchCutoff = 40 000).
  arm A  the only way to serve the request before the list path: 64 one-query
         wv_index_hnsw_flat_search calls (a bitmap and a scan of every row each)
  arm B  one wv_index_hnsw_flat_search_multi_allow call (k_list_dist +
         k_list_heap over the lists' entries)
and the shared-list form: 64 queries under ONE list through the existing call,
option hnsw_list 0 against 1.

The arms alternate after a warm-up of each; a repeat is at least --min-s
seconds of calls on a host clock (every call ends in a stream synchronise),
--repeats repeats per arm; median and min-max per call are reported and the
outputs of the two arms are compared bit for bit in every repeat.  With option
timing = 1 the first launch group's k_list_dist time (device events) is
recorded per shape, and for --chunks the kernel's time per chunks-per-workgroup
setting (option hnsw_list_chunks).

  python tools/bench_hnsw_list.py --comps sq,rq8,bq
  python tools/bench_hnsw_list.py --comps pq --out /tmp/pq.json
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

ap = argparse.ArgumentParser()
ap.add_argument("--comps", default="sq,rq8,bq,pq")
ap.add_argument("--n", type=int, default=1_000_000)
ap.add_argument("--d", type=int, default=768)
ap.add_argument("--nq", type=int, default=64)
ap.add_argument("--k", type=int, default=10)
ap.add_argument("--lens", default="1000,10000,40000")
ap.add_argument("--chunks", default="1,2,4,8", help="hnsw_list_chunks settings timed at the 10 000-id shape")
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--min-s", type=float, default=1.0, help="timed work per repeat and arm")
ap.add_argument("--pq-training-limit", type=int, default=100000)
ap.add_argument("--out", default=os.path.join(REPO, "profiles", "hnsw_list_ab.json"))
args = ap.parse_args()

import numpy as np  # noqa: E402
import torch  # noqa: E402

if not torch.cuda.is_available():
    sys.exit("bench_hnsw_list.py needs a GPU")

import weaviate_amd as wv  # noqa: E402
from weaviate_amd import _lib  # noqa: E402

lib = _lib.load()
dev = torch.device("cuda", 0)
n, d, nq, k = args.n, args.d, args.nq, args.k
lens = [int(x) for x in args.lens.split(",")]


def build(comp):
    kw = dict(distance="l2-squared", dims=d, variant="avx256")
    if comp == "sq":
        kw.update(sq=True, rescore_limit=20)
    elif comp == "rq8":
        kw.update(rq={"bits": 8}, rescore_limit=20)
    elif comp == "bq":
        kw["bq"] = True
    else:
        kw["pq"] = {"segments": 96, "centroids": 256, "trainingLimit": args.pq_training_limit, "rescore": True}
    idx = wv.FlatIndex(**kw)
    idx.reserve(n)
    chunk = 250_000
    stage = torch.empty((min(chunk, n), d), dtype=torch.float32, device=dev)
    for r0 in range(0, n, chunk):
        m = min(chunk, n - r0)
        _lib.check(lib.wv_gen_device(0, 0, 1, r0, m, d, stage.data_ptr(), None))
        _lib.check(lib.wv_index_add_range_device(idx._h, r0, stage.data_ptr(), m, d))
    del stage
    if comp == "sq":
        idx.sq_fit(100000)
    elif comp == "pq":
        idx.pq_fit(seed=9)
    return idx


def same(a, b):
    return bool(np.array_equal(a[2], b[2]) and np.array_equal(a[0], b[0]) and
                np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)))


def ab(arms, label):
    """arms: {name: fn -> (ids, dists, counts)}; alternating repeats -> stats per arm"""
    names = list(arms)
    reps, ref = {}, None
    ok = True
    for a in names:  # warm-up of each arm; its time sizes the repeat
        arms[a]()
        t0 = time.perf_counter()
        out = arms[a]()
        w = time.perf_counter() - t0
        reps[a] = max(1, int(np.ceil(args.min_s / max(w, 1e-6))))
        ref = out if ref is None else ref
        ok = ok and same(ref, out)
    ms = {a: [] for a in names}
    for _ in range(args.repeats):
        for a in names:
            t0 = time.perf_counter()
            for _ in range(reps[a]):
                out = arms[a]()
            ms[a].append((time.perf_counter() - t0) / reps[a] * 1e3)
            ok = ok and same(ref, out)
    row = {"shape": label, "same_results": ok}
    for a in names:
        row[a] = {"median_ms": round(statistics.median(ms[a]), 3), "min_ms": round(min(ms[a]), 3),
                  "max_ms": round(max(ms[a]), 3), "calls_per_repeat": reps[a]}
    print(json.dumps(row), flush=True)
    return row


record = {"device": torch.cuda.get_device_name(0), "n": n, "d": d, "nq": nq, "k": k,
          "timing": "host clock around synchronous calls, per request of nq queries; >= min_s per repeat",
          "min_s": args.min_s, "repeats": args.repeats, "compressors": {}}
q = torch.empty((nq, d), dtype=torch.float32, device=dev)
_lib.check(lib.wv_gen_device(0, 0, 2, 0, nq, d, q.data_ptr(), None))
queries = q.cpu().numpy()
rng = np.random.default_rng(11)
for comp in args.comps.split(","):
    idx = build(comp)
    rec = {"own_lists": [], "shared_list": [], "kernel_ms": [], "chunks": []}
    for L in lens:
        allows = [wv.AllowList(rng.choice(n, L, replace=False)) for _ in range(nq)]

        def arm_a():
            rows = [idx.hnsw_flat_search(queries[i:i + 1], k, allow=allows[i]) for i in range(nq)]
            return tuple(np.concatenate([r[j] for r in rows]) for j in range(3))

        def arm_b():
            return idx.hnsw_flat_search_multi_allow(queries, k, allows)

        row = ab({"A_one_query_calls": arm_a, "B_multi_allow": arm_b}, {"comp": comp, "list_len": L})
        row["B_slowest_faster_than_A_fastest"] = row["B_multi_allow"]["max_ms"] < row["A_one_query_calls"]["min_ms"]
        rec["own_lists"].append(row)
        # kernel level: the first group's k_list_dist (device events, option timing)
        idx.set_option("timing", 1)
        arm_b()
        st = idx.stats()
        rec["kernel_ms"].append({"list_len": L, "k_list_dist_ms": round(st["last_select_ms"], 4),
                                 "entries": int(st["last_scan_rows"])})
        if L == 10000:
            for c in [int(x) for x in args.chunks.split(",")]:
                idx.set_option("hnsw_list_chunks", c)
                arm_b()
                t = [0.0] * 5
                for i in range(5):
                    arm_b()
                    t[i] = idx.stats()["last_select_ms"]
                rec["chunks"].append({"hnsw_list_chunks": c, "k_list_dist_ms_median": round(statistics.median(t), 4),
                                      "min": round(min(t), 4), "max": round(max(t), 4)})
            idx.set_option("hnsw_list_chunks", 0)
        idx.set_option("timing", 0)
        # one list for the whole batch: the existing call, option hnsw_list 0 / 1
        shared = allows[0]

        def one_list(v):
            def f():
                idx.set_option("hnsw_list", v)
                try:
                    return idx.hnsw_flat_search(queries, k, allow=shared)
                finally:
                    idx.set_option("hnsw_list", 0)
            return f

        rec["shared_list"].append(ab({"hnsw_list_0": one_list(0), "hnsw_list_1": one_list(1)},
                                     {"comp": comp, "list_len": L, "one_list_for": nq}))
    print(json.dumps({"comp": comp, "kernel_ms": rec["kernel_ms"], "chunks": rec["chunks"]}), flush=True)
    record["compressors"][comp] = rec
    idx.close()
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(record, f, indent=1)
    f.write("\n")
