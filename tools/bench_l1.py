"""A/B of the two manhattan all-rows kernels in one process: option l1_tile = 0
(the lane-per-pair k_exact_rows<MANHATTAN>) against l1_tile = 1 (the
register-tiled k_l1_rows), alternating, each after a warm-up call of its own,
timed with device events over at least --min-s seconds of work per arm.

The corpus is generated on the device (wv_gen_device).  A row per (n, d, B)
gives ms per batch for each arm (the whole search call: query preparation, the
all-rows kernel and the heap replay) and, for the tiled kernel, its share of
the VALU floor: 2 * B * n * d lane-operations (one v_sub_f32 and one
v_add_f32 per element pair) over the non-packed f32 vector rate of the MI355X,
256 CUs x 64 lanes x 2.4 GHz = 39.3e12 lane-operations per second.

  python tools/bench_l1.py                       # every shape of the record
  python tools/bench_l1.py --shapes 1000000x128x64 --out /tmp/x.json
"""
import argparse
import json
import math
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

SHAPES = "1000000x128x1,1000000x128x8,1000000x128x64,1000000x128x1024,1000000x768x256"
VALU_RATE = 256 * 64 * 2.4e9  # non-packed f32 lane-operations per second

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default=SHAPES, help="comma list of NxDxB")
ap.add_argument("--k", type=int, default=10)
ap.add_argument("--min-s", type=float, default=1.0, help="timed work per arm")
ap.add_argument("--out", default=os.path.join(REPO, "profiles", "l1_tile_ab.json"))
args = ap.parse_args()

import torch  # noqa: E402

if not torch.cuda.is_available():
    sys.exit("bench_l1.py needs a GPU")

import weaviate_amd as wv  # noqa: E402
from weaviate_amd import _lib  # noqa: E402

lib = _lib.load()
dev = torch.device("cuda", 0)
shapes = [tuple(int(x) for x in s.split("x")) for s in args.shapes.split(",")]
rows = []
idx = None
cur = None
for n, d, B in shapes:
    if cur != (n, d):
        if idx is not None:
            idx.close()
        idx = wv.FlatIndex(distance="manhattan", dims=d, variant="avx256")
        idx.reserve(n)
        chunk = 250_000
        stage = torch.empty((min(chunk, n), d), dtype=torch.float32, device=dev)
        for r0 in range(0, n, chunk):
            m = min(chunk, n - r0)
            _lib.check(lib.wv_gen_device(0, 0, 1, r0, m, d, stage.data_ptr(), None))
            _lib.check(lib.wv_index_add_range_device(idx._h, r0, stage.data_ptr(), m, d))
        del stage
        cur = (n, d)
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
    reps = {}
    out = {}
    for tile in (0, 1):  # warm-up of each arm; its time sizes the timed loop
        idx.set_option("l1_tile", tile)
        w = timed(1)
        reps[tile] = max(1, math.ceil(args.min_s * 1e3 / max(w, 1e-3)))
        out[tile] = (oi.cpu().clone(), od.cpu().clone(), on.cpu().clone())
        print(json.dumps({"shape": [n, d, B], "l1_tile": tile, "warmup_ms": round(w, 3), "reps": reps[tile]}),
              flush=True)
    rounds = 2 if max(reps.values()) > 1 else 1  # a batch of seconds is timed once per arm
    for _ in range(rounds):
        for tile in (0, 1):
            idx.set_option("l1_tile", tile)
            ms[tile].append(timed(max(1, reps[tile] // rounds)))
            print(json.dumps({"shape": [n, d, B], "l1_tile": tile, "ms": round(ms[tile][-1], 3)}), flush=True)
    idx.set_option("l1_tile", -1)
    same = all(bool(torch.equal(out[0][j], out[1][j])) for j in range(3))
    simple, tiled = min(ms[0]), min(ms[1])
    floor_ms = 2.0 * B * n * d / VALU_RATE * 1e3
    rows.append({"n": n, "d": d, "B": B, "k": args.k, "simple_ms": round(simple, 3), "tiled_ms": round(tiled, 3),
                 "speedup": round(simple / tiled, 3), "valu_floor_ms": round(floor_ms, 3),
                 "tiled_share_of_floor": round(floor_ms / tiled, 4), "rounds_simple_ms": [round(x, 3) for x in ms[0]],
                 "rounds_tiled_ms": [round(x, 3) for x in ms[1]], "same_results": same})
    print(json.dumps(rows[-1]), flush=True)
if idx is not None:
    idx.close()
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump({"device": torch.cuda.get_device_name(0), "valu_rate_lane_ops_per_s": VALU_RATE,
               "timing": "device events around the whole search call, best round", "rows": rows}, f, indent=1)
    f.write("\n")
