"""GPU parity of the two slot schedules of the paired int8 block-key kernel
(k_q8_blockkey, option q8_sched: 1 = the seamless ring, 0 = the in-order slot
loop).  The seamless ring moves the slot's barrier and DMA
issue, wraps the fragment prefetch into the next slot and defers the second
block's reduction; the keys must not change by a bit.

The other q8 tests run about 20k rows over 128 spans of at most 3 slots, which
never reaches the loop's steady state (t >= 2 and t + 2 < nsteps); the `spans`
option does: 314 slots in 1 .. 314 spans give 314, 5, 4, 3, 2 and 1 slots per
span.  n = 20037 ends in a slot of 5 rows in block 0 and an empty block 1."""
import numpy as np
import pytest

from test_gpu_flat import assert_same, build_pair, gen

pytestmark = pytest.mark.gpu

ROUTE_INT8, ROUTE_PQ_INT8 = 3, 8

SHAPES = {
    "cosine768": ("cosine", 0, 768, 10),
    "l2int512": ("l2-squared", 1, 512, 100),  # integer data: exact codes, ties
    "dot640": ("dot", 0, 640, 10),
}
N_FULL = 20037
SPANS = [1, 63, 79, 105, 157, 314]
NQ_PLAIN, NQ_LIVE = 512, 300  # whole query groups / a last group with padding waves (LIVE)

_cache = {}


@pytest.fixture(scope="module", autouse=True)
def _close_indexes():
    yield
    for v in _cache.values():
        v["idx"].close()
    _cache.clear()


def setup(wv, oracle, shape, n):
    """One index, oracle and query set per (shape, n), shared by its cases."""
    key = (shape, n)
    if key not in _cache:
        metric, kind, d, k = SHAPES[shape]
        data = gen(oracle, kind, 91, n, d)
        queries = gen(oracle, kind, 92, NQ_PLAIN, d)
        idx, orc = build_pair(wv, oracle, metric, "avx256", data)
        idx.set_option("q8_gemv", 0)
        _cache[key] = {"idx": idx, "orc": orc, "queries": queries, "k": k, "ref": {}}
    return _cache[key]


def search_arm(idx, queries, k, sched, sample):
    idx.set_option("q8_sched", sched)
    res = idx.search_by_vector_batch(queries, k)
    assert idx.stats()["last_route"] == ROUTE_INT8
    keys = [idx.debug_blockkeys(q)[0] for q in sample]
    return res, keys


def assert_arms_equal(old, new, ctx):
    (res0, keys0), (res1, keys1) = old, new
    for a, b, what in zip(res0, res1, ("ids", "dists", "counts")):
        np.testing.assert_array_equal(np.asarray(a).view(np.uint8), np.asarray(b).view(np.uint8),
                                      err_msg=f"{ctx}: {what}")
    for i, (a, b) in enumerate(zip(keys0, keys1)):
        assert a.size == b.size
        np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32), err_msg=f"{ctx}: block keys, sample {i}")


def run_case(wv, oracle, shape, n, nq, spans):
    c = setup(wv, oracle, shape, n)
    idx, k = c["idx"], c["k"]
    queries = c["queries"][:nq]
    sample = [0, 31, 32, 255, 256, nq - 1]
    idx.set_option("spans", spans)
    old = search_arm(idx, queries, k, 0, sample)
    new = search_arm(idx, queries, k, 1, sample)
    ctx = f"{shape} n={n} nq={nq} spans={spans}"
    assert_arms_equal(old, new, ctx)
    ids, dists, counts = new[0]
    for qi in range(0, nq, 10):
        if qi not in c["ref"]:
            c["ref"][qi] = c["orc"].search(queries[qi], k)
        assert_same(c["ref"][qi], ids[qi, :counts[qi]], dists[qi, :counts[qi]], ctx=f"{ctx} q{qi}")


@pytest.mark.parametrize("spans", SPANS)
@pytest.mark.parametrize("nq", [NQ_PLAIN, NQ_LIVE])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_sched_arms_equal_every_span_length(wv, oracle, shape, nq, spans):
    run_case(wv, oracle, shape, N_FULL, nq, spans)


@pytest.mark.parametrize("n", [40, 100])  # a whole corpus of 1 and 2 slots
@pytest.mark.parametrize("nq", [NQ_PLAIN, NQ_LIVE])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_sched_arms_equal_tiny_corpus(wv, oracle, shape, nq, n):
    run_case(wv, oracle, shape, n, nq, 0)


@pytest.mark.parametrize("nq", [NQ_PLAIN, NQ_LIVE])
def test_sched_arms_equal_with_deleted_blocks(wv, oracle, nq):
    """Partially valid and fully invalid blocks as block 1 of one slot and block
    0 of the next -- the valid word and scale the seamless ring carries across
    the slot boundary -- at the last block of a span and the first of the next
    (63 spans of 5 slots = 10 blocks) and in one long span.  A block without a
    valid row keys +inf in both arms."""
    metric, kind, d, k = SHAPES["cosine768"]
    n = N_FULL
    data = gen(oracle, kind, 93, n, d)
    queries = gen(oracle, kind, 94, nq, d)
    idx, orc = build_pair(wv, oracle, metric, "avx256", data)
    idx.set_option("q8_gemv", 0)
    rows = lambda b, lo=0, hi=32: list(range(32 * b + lo, 32 * b + hi))
    # (block 1 of a slot, block 0 of the next): (gone, partial) over a span end,
    # (partial, gone) and (gone, gone) inside spans, (partial, partial) over a span end
    gone = rows(9) + rows(10, 0, 21) + rows(21, 3, 20) + rows(22) + rows(33) + rows(34) + rows(49, 31) + rows(50, 0, 1)
    empty = [9, 22, 33, 34]
    idx.delete(*gone)
    orc.delete(gone)
    sample = [0, 31, 32, 255, 256, nq - 1]
    for spans in (63, 1):
        idx.set_option("spans", spans)
        old = search_arm(idx, queries, k, 0, sample)
        new = search_arm(idx, queries, k, 1, sample)
        assert_arms_equal(old, new, f"deleted nq={nq} spans={spans}")
        for keys in old[1] + new[1]:
            assert np.isposinf(keys[empty]).all()
            assert np.isfinite(np.delete(keys[: n // 32], empty)).all()
        ids, dists, counts = new[0]
        for qi in range(0, nq, 10):
            assert_same(orc.search(queries[qi], k), ids[qi, :counts[qi]], dists[qi, :counts[qi]],
                        ctx=f"deleted spans={spans} q{qi}")
    idx.close()


def test_sched_arms_equal_pq_int8_route(wv, oracle):
    """The PQ int8 keys (launch_q8_keys, l2 keys over the centred reconstruction
    plane, dpb8 512: the paired kernel) on both schedules: 47 slots in one span
    and in 12 spans of 4."""
    n, d, k = 3000, 400, 10
    data = gen(oracle, 2, 95, n, d)
    idx = wv.FlatIndex(distance="l2-squared", variant="avx256", pq={"segments": 100, "centroids": 32, "rescore": False})
    idx.add_batch(np.arange(n, dtype=np.uint64), data)
    idx.pq_fit(seed=23)
    idx.delete(*range(5, n, 97))
    queries = gen(oracle, 2, 96, 70, d)
    idx.set_option("pq8", 1)
    for spans in (1, 12):
        idx.set_option("spans", spans)
        res = {}
        for sched in (0, 1):
            idx.set_option("q8_sched", sched)
            res[sched] = idx.search_by_vector_batch(queries, k)
            assert idx.stats()["last_route"] == ROUTE_PQ_INT8
        for a, b in zip(res[0], res[1]):
            np.testing.assert_array_equal(np.asarray(a).view(np.uint8), np.asarray(b).view(np.uint8))
    idx.close()
