"""A/B of the two routes of the hnsw flat search over SQ in one process: option
sq_keys = 0 (the distance-matrix route: k_sq_dist + k_replay_scan) against
sq_keys = 1 (k_sq_keys -> k_rq8_sel -> k_sq_cand, flagged queries replayed;
DESIGN §3.10c), alternating in arm pairs, each arm after a warm-up call of its
own, timed with device events around the whole wv_index_hnsw_flat_search call
(host queries in, host results out) over at least --min-s seconds of work per
arm.  Results are compared bit for bit on every row of every cell.

The corpus is generated on the device (wv_gen_device, U[-1, 1)).  A row per
(metric, n, d, B) gives ms per call for each arm (best pair), the spread of the
pairs of the same arm ((max - min) / min) and the share of the queries the new
route flagged and replayed.

  python tools/bench_sq_keys.py                       # every cell of the record
  python tools/bench_sq_keys.py --shapes 30000x128 --batches 8,256 --out /tmp/x.json
"""
import argparse
import json
import math
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default="1000000x768,1000000x128,30000x128", help="comma list of NxD")
ap.add_argument("--batches", default="8,64,256,2048")
ap.add_argument("--metrics", default="l2-squared,dot,cosine")
ap.add_argument("--k", type=int, default=10)
ap.add_argument("--min-s", type=float, default=1.0, help="timed work per arm")
ap.add_argument("--pairs", type=int, default=3, help="arm pairs the timed work is split into")
ap.add_argument("--out", default=os.path.join(REPO, "profiles", "sq_keys_ab.json"))
args = ap.parse_args()

import torch  # noqa: E402

if not torch.cuda.is_available():
    sys.exit("bench_sq_keys.py needs a GPU")

import weaviate_amd as wv  # noqa: E402
from weaviate_amd import _lib  # noqa: E402

lib = _lib.load()
dev = torch.device("cuda", 0)
stream = torch.cuda.current_stream(dev)
rows = []
for shape in args.shapes.split(","):
    n, d = (int(x) for x in shape.split("x"))
    for metric in args.metrics.split(","):
        idx = wv.FlatIndex(distance=metric, dims=d, variant="avx256", sq=True, rescore_limit=20)
        idx.reserve(n)
        chunk = 100_000
        stage = torch.empty((min(chunk, n), d), dtype=torch.float32, device=dev)
        for r0 in range(0, n, chunk):
            m = min(chunk, n - r0)
            _lib.check(lib.wv_gen_device(0, 0, 1, r0, m, d, stage.data_ptr(), None))
            _lib.check(lib.wv_index_add_range_device(idx._h, r0, stage.data_ptr(), m, d))
        del stage
        idx.sq_fit(100_000)
        for B in (int(b) for b in args.batches.split(",")):
            qd = torch.empty((B, d), dtype=torch.float32, device=dev)
            _lib.check(lib.wv_gen_device(0, 0, 2, 0, B, d, qd.data_ptr(), None))
            q = qd.cpu().numpy()

            def timed(reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                for _ in range(reps):
                    idx.hnsw_flat_search(q, args.k)
                e1.record(stream)
                e1.synchronize()
                return e0.elapsed_time(e1) / reps

            ms = {0: [], 1: []}
            reps, out, route, flagged = {}, {}, {}, 0.0
            for arm in (0, 1):  # warm-up of each arm; a second call's time sizes the timed loop
                idx.set_option("sq_keys", arm)
                before = idx.stats()["replayed_queries"]
                out[arm] = idx.hnsw_flat_search(q, args.k)
                if arm == 1:
                    flagged = (idx.stats()["replayed_queries"] - before) / B
                route[arm] = _lib.ROUTES[idx.stats()["last_route"]] if arm else "matrix"
                w = timed(1)
                reps[arm] = max(1, math.ceil(args.min_s * 1e3 / max(w, 1e-3) / args.pairs))
            for _ in range(args.pairs):
                for arm in (0, 1):
                    idx.set_option("sq_keys", arm)
                    ms[arm].append(timed(reps[arm]))
            idx.set_option("sq_keys", -1)
            same = all(bool((out[0][j].view("u4") == out[1][j].view("u4")).all()) for j in (1, 2)) and \
                bool((out[0][0] == out[1][0]).all())
            base, keys = min(ms[0]), min(ms[1])
            rows.append({"metric": metric, "n": n, "d": d, "B": B, "k": args.k, "route_keys": route[1],
                         "matrix_ms": round(base, 3), "keys_ms": round(keys, 3), "speedup": round(base / keys, 3),
                         "spread_matrix": round(max(ms[0]) / base - 1, 4), "spread_keys": round(max(ms[1]) / keys - 1, 4),
                         "flagged_share": round(flagged, 4),
                         "pairs_matrix_ms": [round(x, 3) for x in ms[0]], "pairs_keys_ms": [round(x, 3) for x in ms[1]],
                         "reps": [reps[0], reps[1]], "same_results": same})
            print(json.dumps(rows[-1]), flush=True)
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:  # rewritten after every cell: a cut-off run keeps its finished cells
                json.dump({"device": torch.cuda.get_device_name(0),
                           "timing": "device events around the whole hnsw_flat_search call (host in, host out), "
                                     "arm pairs alternating, best pair; ef auto (limit 100), rescore_limit 20",
                           "rows": rows}, f, indent=1)
                f.write("\n")
        idx.close()
