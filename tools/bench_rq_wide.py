"""A/B of the rq-8 / rq-1 routes above 1024 rotated dims in one process: option
rq_wide = 0 (the distance-matrix route: k_rq8_dist / k_rq1_dist + k_replay_scan)
against rq_wide = 1 (k_rq8_keys_cp -> k_rq8_sel -> k_rq8_cand -> k_rq8_replay,
DESIGN §3.7c), alternating in arm pairs, each arm after a warm-up call of its
own, timed with device events over at least --min-s seconds of work per arm.
Results are compared bit for bit in every cell.

The corpus is generated on the device (wv_gen_device).  A row per (bits, n, d,
B) gives ms per batch for each arm: the whole search call (best pair, and the
spread of the pairs: (max - min) / min per arm) and the first pass alone
(option timing = 1: the key kernel, or the first group's distance kernel).  For
the key kernel it also gives the share of the int8 MFMA peak of the MI355X:
2 * B * n * D operations (D the rotated width) over 256 CUs x 4 SIMDs x 2048 ops
per cycle x 2.4 GHz = 5.03e15 per second.

  python tools/bench_rq_wide.py                       # every cell of the record
  python tools/bench_rq_wide.py --bits 8 --shapes 1000000x1536x256 --out /tmp/x.json
"""
import argparse
import json
import math
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

SHAPES = ",".join(f"1000000x{d}x{b}" for d in (1536, 3072, 4000) for b in (256, 2048))
MFMA_RATE = 256 * 4 * 2048 * 2.4e9  # int8 operations per second

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default=SHAPES, help="comma list of NxDxB")
ap.add_argument("--bits", default="8,1")
ap.add_argument("--k", type=int, default=10)
ap.add_argument("--rescore", type=int, default=200)
ap.add_argument("--min-s", type=float, default=1.0, help="timed work per arm")
ap.add_argument("--pairs", type=int, default=3, help="arm pairs the timed work is split into")
ap.add_argument("--out", default=os.path.join(REPO, "profiles", "rq_wide_ab.json"))
args = ap.parse_args()

import torch  # noqa: E402

if not torch.cuda.is_available():
    sys.exit("bench_rq_wide.py needs a GPU")

import weaviate_amd as wv  # noqa: E402
from weaviate_amd import _lib  # noqa: E402

lib = _lib.load()
dev = torch.device("cuda", 0)
shapes = [tuple(int(x) for x in s.split("x")) for s in args.shapes.split(",")]
rows = []
for bits in [int(b) for b in args.bits.split(",")]:
    idx = None
    cur = None
    for n, d, B in shapes:
        if cur != (n, d):
            if idx is not None:
                idx.close()
            idx = wv.FlatIndex(distance="cosine", dims=d, variant="avx256", rq={"bits": bits}, rescore_limit=args.rescore)
            idx.reserve(n)
            chunk = 100_000
            stage = torch.empty((min(chunk, n), d), dtype=torch.float32, device=dev)
            for r0 in range(0, n, chunk):
                m = min(chunk, n - r0)
                _lib.check(lib.wv_gen_device(0, 0, 1, r0, m, d, stage.data_ptr(), None))
                _lib.check(lib.wv_index_add_range_device(idx._h, r0, stage.data_ptr(), m, d))
            del stage
            cur = (n, d)
        D = idx.rq_info()["output_dim"]
        q = torch.empty((B, d), dtype=torch.float32, device=dev)
        _lib.check(lib.wv_gen_device(0, 0, 2, 0, B, d, q.data_ptr(), None))
        oi = torch.empty((B, args.k), dtype=torch.int64, device=dev)
        od = torch.empty((B, args.k), dtype=torch.float32, device=dev)
        on = torch.empty(B, dtype=torch.int32, device=dev)
        stream = torch.cuda.current_stream(dev)

        def run():
            _lib.check(lib.wv_index_search_device(idx._h, q.data_ptr(), B, d, args.k, 0, oi.data_ptr(), od.data_ptr(),
                                                  on.data_ptr(), None, stream.cuda_stream))

        def timed(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(reps):
                run()
            e1.record(stream)
            e1.synchronize()
            return e0.elapsed_time(e1) / reps

        ms = {0: [], 1: []}
        reps, out, route, first = {}, {}, {}, {}
        for arm in (0, 1):  # warm-up of each arm; its time sizes the timed loop
            idx.set_option("rq_wide", arm)
            w = timed(1)
            reps[arm] = max(1, math.ceil(args.min_s * 1e3 / max(w, 1e-3) / args.pairs))
            out[arm] = (oi.cpu().clone(), od.cpu().clone(), on.cpu().clone())
            route[arm] = idx.stats()["last_route"]
            idx.set_option("timing", 1)  # the first pass alone, by the index's own events
            run()
            torch.cuda.synchronize()
            first[arm] = idx.stats()["last_select_ms"]
            idx.set_option("timing", 0)
            print(json.dumps({"bits": bits, "shape": [n, d, B], "rq_wide": arm, "route": route[arm],
                              "warmup_ms": round(w, 3), "first_pass_ms": round(first[arm], 3), "reps": reps[arm]}),
                  flush=True)
        for _ in range(args.pairs):
            for arm in (0, 1):
                idx.set_option("rq_wide", arm)
                ms[arm].append(timed(reps[arm]))
        idx.set_option("rq_wide", -1)
        same = all(bool(torch.equal(out[0][j], out[1][j])) for j in range(3))
        base, wide = min(ms[0]), min(ms[1])
        peak_ms = 2.0 * B * n * D / MFMA_RATE * 1e3
        rows.append({"bits": bits, "n": n, "d": d, "D": D, "B": B, "k": args.k, "rescore": args.rescore,
                     "route_base": route[0], "route_wide": route[1], "base_ms": round(base, 3),
                     "wide_ms": round(wide, 3), "speedup": round(base / wide, 3),
                     "spread_base": round(max(ms[0]) / base - 1, 4), "spread_wide": round(max(ms[1]) / wide - 1, 4),
                     "base_dist_pass_ms": round(first[0], 3), "wide_key_pass_ms": round(first[1], 3),
                     "key_pass_share_of_mfma_peak": round(peak_ms / max(first[1], 1e-6), 4),
                     "pairs_base_ms": [round(x, 3) for x in ms[0]], "pairs_wide_ms": [round(x, 3) for x in ms[1]],
                     "same_results": same})
        print(json.dumps(rows[-1]), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:  # rewritten after every cell: a cut-off run keeps its finished cells
            json.dump({"device": torch.cuda.get_device_name(0), "int8_mfma_ops_per_s": MFMA_RATE,
                       "timing": "device events around the whole search call, arm pairs alternating, best pair; "
                                 "first pass from option timing",
                       "rows": rows}, f, indent=1)
            f.write("\n")
    if idx is not None:
        idx.close()
