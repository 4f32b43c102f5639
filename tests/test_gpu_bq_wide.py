"""GPU: BQ block minima from the packed codes (k_bq_packmin, option bq_pack,
route 13) and the 32-row replay's arm for 33-64 code words:
minima and results equal the bq_pack = 0 arm's byte for byte and the oracle's."""
import numpy as np
import pytest
import torch

from test_gpu_flat import assert_same, build_bq_pair, gen

pytestmark = pytest.mark.gpu

ROUTE_BQ_INT8, ROUTE_BQ_VALU, ROUTE_BQ_PACKED = 6, 7, 13


def same_bytes(got, ref, ctx=""):
    for a, b in zip(got, ref):
        np.testing.assert_array_equal(np.asarray(a).view(np.uint8), np.asarray(b).view(np.uint8), err_msg=ctx)


def check_arms(wv, idx, orc, queries, k, probe, every, ref_route, allow=None, ctx=""):
    """the batch under bq_pack = 1 and = 0: routes, the probed queries' minima
    (on 256-row blocks), results; every `every`-th query against the oracle"""
    res = {}
    for pack in (1, 0):
        idx.set_option("bq_pack", pack)
        out = idx.search_by_vector_batch(queries, k, allow=None if allow is None else wv.AllowList(allow))
        res[pack] = (out, idx.stats()["last_route"], [idx.debug_bqmin(q) for q in probe])
    idx.set_option("bq_pack", -1)
    (got, route, mins), (ref, rroute, rmins) = res[1], res[0]
    assert route == ROUTE_BQ_PACKED and rroute == ref_route
    for q, m, v in zip(probe, mins, rmins):
        np.testing.assert_array_equal(m[: v.size], v, err_msg=f"{ctx} block minima q{q}")
        assert np.all(np.isinf(m[v.size:]))
    same_bytes(got, ref, ctx)
    for q in range(0, len(queries), every):
        assert_same(orc.search(queries[q], k, allow=allow), got[0][q, :got[2][q]], got[1][q, :got[2][q]], f"{ctx} q{q}")
    return got


@pytest.mark.parametrize("metric,kind,n,d", [
    ("cosine", 0, 5077, 1600),      # 25 words, the first width past the plane; ragged last block, odd block count
    ("l2-squared", 0, 4000, 2100),  # 33 words, 52 bits in the last; the first width of the replay's chunked arm
    ("dot", 0, 3005, 3072),         # 48 words
    ("cosine", 1, 2100, 4096),      # 64 words; all-positive data: every code 0, every distance ties
])
def test_bq_packed_minima_and_results(wv, oracle, metric, kind, n, d):
    data = gen(oracle, kind, 183, n, d)
    queries = gen(oracle, kind, 184, 300, d)  # full query groups plus a ragged tail
    idx, orc = build_bq_pair(wv, oracle, metric, "avx256", data, 64)
    idx.search_by_vector_batch(queries[:1], 10)
    assert idx.stats()["last_route"] == ROUTE_BQ_PACKED  # auto takes 25-64 words
    check_arms(wv, idx, orc, queries, 10, (0, 150, 299), 12, ROUTE_BQ_VALU, ctx=f"d={d}")
    check_arms(wv, idx, orc, queries[7:8], 10, (0,), 1, ROUTE_BQ_VALU, ctx=f"d={d} B=1")
    idx.close()


def test_bq_packed_deletes_upserts_allow(wv, oracle):
    n, d, k = 3000, 3072, 10
    data = gen(oracle, 0, 185, n, d)
    idx, orc = build_bq_pair(wv, oracle, "cosine", "avx512", data, 64)
    # every 7th id, one whole 32-row block and one whole 256-row span
    dele = np.unique(np.concatenate([np.arange(0, n, 7), np.arange(96, 128), np.arange(512, 768)])).astype(np.uint64)
    idx.delete(*dele)
    orc.delete(dele)
    up = gen(oracle, 0, 186, 300, d)
    upids = np.arange(2000, 2300, dtype=np.uint64)
    idx.add_batch(upids, up)
    orc.add_batch(upids, up)
    queries = gen(oracle, 0, 187, 64, d)
    for allow in (None, np.arange(50, 2900, 3, dtype=np.uint64)):
        check_arms(wv, idx, orc, queries, k, (5,), 8, ROUTE_BQ_VALU, allow=allow, ctx=f"allow={allow is not None}")
    idx.close()


@pytest.mark.parametrize("d,ref_route", [(100, ROUTE_BQ_VALU), (768, ROUTE_BQ_INT8)])
def test_bq_packed_forced_at_narrow_widths(wv, oracle, d, ref_route):
    """bq_pack = 1 below 25 words (2 words with a partial last one, 12 words):
    the default route's minima and results"""
    n = 4000 + 21
    data = gen(oracle, 0, 188, n, d)
    queries = gen(oracle, 0, 189, 100, d)
    idx, orc = build_bq_pair(wv, oracle, "l2-squared", "avx256", data, 40)
    idx.search_by_vector_batch(queries, 10)
    assert idx.stats()["last_route"] == ref_route  # auto leaves these widths alone
    check_arms(wv, idx, orc, queries, 10, (0, 99), 12, ref_route, ctx=f"d={d}")
    idx.close()


def test_bq_packed_past_64_words_keeps_the_valu_route(wv, oracle):
    n, d = 1500, 4100  # 65 words
    data = gen(oracle, 0, 190, n, d)
    queries = gen(oracle, 0, 191, 24, d)
    idx, orc = build_bq_pair(wv, oracle, "cosine", "avx256", data, 30)
    idx.set_option("bq_pack", 1)
    ids, dists, counts = idx.search_by_vector_batch(queries, 10)
    assert idx.stats()["last_route"] == ROUTE_BQ_VALU
    for q in range(len(queries)):
        assert_same(orc.search(queries[q], 10), ids[q, :counts[q]], dists[q, :counts[q]], f"q{q}")
    idx.close()


def test_bq_packed_multi_allow_equals_one_query_calls(wv, oracle):
    """the replay's PQA arm at 33 words: 24 queries, each under its own list"""
    n, d, k, nq = 4000, 2100, 10, 24
    data = gen(oracle, 0, 192, n, d)
    queries = gen(oracle, 0, 193, nq, d)
    idx, _ = build_bq_pair(wv, oracle, "l2-squared", "avx256", data, 30)
    rng = np.random.default_rng(7)
    allows = [wv.AllowList(rng.choice(n, 20 + 150 * i, replace=False)) for i in range(nq)]
    allows[3], allows[11] = wv.AllowList(), None  # the empty list, an unlisted query
    idx.set_option("bq_pack", 0)
    one = [idx.search_by_vector_batch(queries[i:i + 1], k, allow=allows[i]) for i in range(nq)]
    idx.set_option("bq_pack", 1)
    b0 = idx.stats()["batches"]
    ids, dists, counts = idx.search_by_vector_batch_multi_allow(queries, k, allows)
    assert idx.stats()["batches"] - b0 == 1 and idx.stats()["last_route"] == ROUTE_BQ_PACKED
    assert counts[3] == 0
    for i in range(nq):  # the entries past a row's count are not written
        m = int(one[i][2][0])
        same_bytes((ids[i, :m], dists[i, :m], counts[i:i + 1]), (one[i][0][0, :m], one[i][1][0, :m], one[i][2]), f"q{i}")
    idx.close()


def test_bq_packed_sharded_chain_and_record(wv, oracle):
    """33 words over 3 shards: the chained replay equals the single index, and
    the recording replay (REC arm) records the bq_pack = 0 arm's insertions"""
    from weaviate_amd.sharded import GpuBQShardBackend
    shards, n, d, k, rl = 3, 3000, 2100, 10, 64
    data = gen(oracle, 0, 194, n, d)
    q = torch.from_numpy(gen(oracle, 0, 195, 64, d)).to("cuda:0")
    per = n // shards
    backs = []
    for r in range(shards):
        idx = wv.FlatIndex(distance="cosine", bq=True, rescore_limit=rl, id_base=r * per, variant="avx256")
        idx.add_batch(np.arange(r * per, (r + 1) * per, dtype=np.uint64), data[r * per:(r + 1) * per])
        backs.append(GpuBQShardBackend(idx, 0))
    empty = (torch.zeros((64, rl), dtype=torch.int64, device="cuda:0"),
             torch.zeros((64, rl), dtype=torch.float32, device="cuda:0"), torch.zeros(64, dtype=torch.int32, device="cuda:0"))
    res = {}
    for pack in (1, 0):
        state = None
        for r, b in enumerate(backs):
            b.index.set_option("bq_pack", pack)
            b.bq_begin(q, k)
            state = b.bq_replay(state, r == shards - 1)
        ids, _, ln = state
        E_all = torch.stack([b.bq_rescore(ids, ln) for b in backs])
        rec = backs[1].bq_replay_record(empty, per)
        torch.cuda.synchronize()
        res[pack] = [t.cpu().numpy() for t in backs[0].bq_final(shards, per, ids, ln, E_all) + rec]
        assert backs[0].index.stats()["last_route"] == (ROUTE_BQ_PACKED if pack else ROUTE_BQ_VALU)
    rn = res[1][5]
    assert 0 < rn.min() and rn.max() <= per
    np.testing.assert_array_equal(rn, res[0][5])
    for a, b in zip(res[1][3:5], res[0][3:5]):
        for i in range(64):
            np.testing.assert_array_equal(a[i, :rn[i]].view(np.uint32), b[i, :rn[i]].view(np.uint32), err_msg=f"record q{i}")
    single = wv.FlatIndex(distance="cosine", bq=True, rescore_limit=rl, variant="avx256")
    single.add_batch(np.arange(n, dtype=np.uint64), data)
    si, sd, sn = single.search_by_vector_batch(q.cpu().numpy(), k)
    oi, od, on = res[1][:3]
    np.testing.assert_array_equal(on, sn)
    np.testing.assert_array_equal(oi.astype(np.uint64), si)
    np.testing.assert_array_equal(od.view(np.uint32), sd.view(np.uint32))
    for b in backs:
        b.index.close()
    single.close()
