"""A/B of the BQ block-minima routes on wide codes in one process: option
bq_pack = 0 (the stored-plane / VALU / generic kernels, whichever the width
takes) against bq_pack = 1 (k_bq_packmin over the packed codes and, above 32
words, the 32-row replay's chunked arm), alternating, each after a warm-up call
of its own, timed with device events over at least --min-s seconds of work per
arm.  Results are compared bit for bit in every cell.

The corpus is generated on the device (wv_gen_device).  A row per (n, d, B)
gives ms per batch for each arm: the whole search call, the block-minima pass
(option timing = 1, one extra call per arm) and the R-heap replay (the sharded
entry points: wv_index_bq_begin once, then wv_index_bq_replay timed alone).
For the packed kernel it also gives the share of the int8 MFMA peak of the
MI355X: 2 * B * n * 64 * words operations over 256 CUs x 4 SIMDs x 2048 ops
per cycle x 2.4 GHz = 5.03e15 per second.

  python tools/bench_bq_wide.py                      # every shape of the record
  python tools/bench_bq_wide.py --shapes 1000000x4096x256 --out /tmp/x.json
  python tools/bench_bq_wide.py --parent             # in a checkout without the option

--parent times the default route only and never names the option: run from a
checkout of the parent commit it gives the baseline rows ("parent_ms", ...)
that the bq_pack = 0 arm is compared with.
"""
import argparse
import json
import math
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

SHAPES = ",".join(f"1000000x{d}x{b}" for d in (2048, 3072, 4096) for b in (16, 256, 2048)) + ",1000000x1536x2048"
MFMA_RATE = 256 * 4 * 2048 * 2.4e9  # int8 operations per second

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default=SHAPES, help="comma list of NxDxB")
ap.add_argument("--k", type=int, default=10)
ap.add_argument("--rescore", type=int, default=200)
ap.add_argument("--min-s", type=float, default=1.0, help="timed work per arm")
ap.add_argument("--parent", action="store_true", help="default route only, no bq_pack option (parent commit)")
ap.add_argument("--out", default=os.path.join(REPO, "profiles", "bq_packed_ab.json"))
args = ap.parse_args()

import torch  # noqa: E402

if not torch.cuda.is_available():
    sys.exit("bench_bq_wide.py needs a GPU")

import weaviate_amd as wv  # noqa: E402
from weaviate_amd import _lib  # noqa: E402
from weaviate_amd.sharded import GpuBQShardBackend  # noqa: E402

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
        idx = wv.FlatIndex(distance="cosine", dims=d, variant="avx256", bq=True, rescore_limit=args.rescore)
        idx.reserve(n)
        chunk = 100_000
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

    back = GpuBQShardBackend(idx, 0)

    def timed_replay(reps):
        back.bq_begin(q, args.k)  # codes + minima of the batch; the replay below reads them
        back.bq_replay(None, True)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(reps):
            back.bq_replay(None, True)
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) / reps

    arms = (0,) if args.parent else (0, 1)

    def set_arm(pack):
        if not args.parent:
            idx.set_option("bq_pack", pack)

    ms = {a: [] for a in arms}
    reps, out, route, minima, replay = {}, {}, {}, {}, {}
    for pack in arms:  # warm-up of each arm; its time sizes the timed loop
        set_arm(pack)
        w = timed(1)
        reps[pack] = max(1, math.ceil(args.min_s * 1e3 / max(w, 1e-3)))
        out[pack] = (oi.cpu().clone(), od.cpu().clone(), on.cpu().clone())
        route[pack] = idx.stats()["last_route"]
        idx.set_option("timing", 1)  # the block-minima pass alone, by the index's own events
        run()
        torch.cuda.synchronize()
        minima[pack] = idx.stats()["last_select_ms"]
        idx.set_option("timing", 0)
        replay[pack] = timed_replay(max(1, reps[pack] // 4))
        print(json.dumps({"shape": [n, d, B], "bq_pack": pack, "route": route[pack], "warmup_ms": round(w, 3),
                          "minima_ms": round(minima[pack], 3), "replay_ms": round(replay[pack], 3), "reps": reps[pack]}),
              flush=True)
    rounds = 2 if max(reps.values()) > 1 else 1  # a batch of seconds is timed once per arm
    for _ in range(rounds):
        for pack in arms:
            set_arm(pack)
            ms[pack].append(timed(max(1, reps[pack] // rounds)))
            print(json.dumps({"shape": [n, d, B], "bq_pack": pack, "ms": round(ms[pack][-1], 3)}), flush=True)
    words = (d + 63) // 64
    if args.parent:
        rows.append({"n": n, "d": d, "words": words, "B": B, "k": args.k, "rescore": args.rescore,
                     "route_parent": route[0], "parent_ms": round(min(ms[0]), 3),
                     "parent_minima_ms": round(minima[0], 3), "parent_replay_ms": round(replay[0], 3),
                     "rounds_parent_ms": [round(x, 3) for x in ms[0]]})
        print(json.dumps(rows[-1]), flush=True)
        with open(args.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "rows": rows}, f, indent=1)
            f.write("\n")
        continue
    idx.set_option("bq_pack", -1)
    same = all(bool(torch.equal(out[0][j], out[1][j])) for j in range(3))
    base, pack = min(ms[0]), min(ms[1])
    peak_ms = 2.0 * B * n * 64 * words / MFMA_RATE * 1e3
    rows.append({"n": n, "d": d, "words": words, "B": B, "k": args.k, "rescore": args.rescore,
                 "route_base": route[0], "route_packed": route[1], "base_ms": round(base, 3),
                 "packed_ms": round(pack, 3), "speedup": round(base / pack, 3),
                 "base_minima_ms": round(minima[0], 3), "packed_minima_ms": round(minima[1], 3),
                 "base_replay_ms": round(replay[0], 3), "packed_replay_ms": round(replay[1], 3),
                 "packed_minima_share_of_mfma_peak": round(peak_ms / max(minima[1], 1e-6), 4),
                 "rounds_base_ms": [round(x, 3) for x in ms[0]], "rounds_packed_ms": [round(x, 3) for x in ms[1]],
                 "same_results": same})
    print(json.dumps(rows[-1]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:  # rewritten after every cell: a cut-off run keeps its finished cells
        json.dump({"device": torch.cuda.get_device_name(0), "int8_mfma_ops_per_s": MFMA_RATE,
                   "timing": "device events around the whole search call, best round; minima from option timing; "
                             "replay = wv_index_bq_replay alone after one wv_index_bq_begin",
                   "rows": rows}, f, indent=1)
        f.write("\n")
if idx is not None:
    idx.close()
