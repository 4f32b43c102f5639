"""GPU: the manhattan distance (distancer/manhattan.go) -- the provider, the
exact search through both all-rows kernels (l1_tile = 0: the lane-per-pair
k_exact_rows, 1: the register-tiled k_l1_rows), writes and filters, BQ
rescoring and the multi-shard index.

The oracle library knows no manhattan, so the expected distances come from
numpy: np.add.accumulate(|a - b|, dtype=float32) is the reference's one fp32
accumulator advanced in element order.  Tie order comes from oracle.heap_scan
(the reference heap over precomputed distances of rows [0, n) in id order);
under deletes and allow lists the present rows are scanned in id order and the
positions mapped back to ids.  Distances are compared as uint32 bit patterns.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROUTE_L1_TILE = 11  # WV_ROUTE_L1_TILE


def l1(a, b):
    """Sequential fp32 sum of |a - b| over the last axis (broadcasting)."""
    a = np.asarray(a, np.float32)
    b = np.asarray(b, np.float32)
    with np.errstate(invalid="ignore"):
        return np.add.accumulate(np.abs(a - b), axis=-1, dtype=np.float32)[..., -1]


def uniform(seed, *shape):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, size=shape).astype(np.float32)


def expect(oracle, data, ids, q, k):
    """Reference result of one query over rows `data` holding doc ids `ids` (ascending)."""
    pos, dd = oracle.heap_scan(l1(q, data), k)
    return np.asarray(ids, np.uint64)[pos.astype(np.int64)], dd


def check_batch(oracle, got, data, ids, queries, k, tag="", nan_ok=False):
    gi, gd, gn = got
    for i, q in enumerate(queries):
        ei, ed = expect(oracle, data, ids, q, k)
        assert gn[i] == len(ei), f"{tag} q{i} count {gn[i]} != {len(ei)}"
        np.testing.assert_array_equal(gi[i, :gn[i]], ei, err_msg=f"{tag} q{i} ids")
        if nan_ok:
            np.testing.assert_array_equal(gd[i, :gn[i]], ed, err_msg=f"{tag} q{i} dists")  # NaN == NaN
        else:
            np.testing.assert_array_equal(gd[i, :gn[i]].view(np.uint32), ed.view(np.uint32),
                                          err_msg=f"{tag} q{i} dists")


def make_index(wv, data, l1_tile=None, **kw):
    idx = wv.FlatIndex(distance="manhattan", variant="avx256", **kw)
    idx.add_batch(np.arange(data.shape[0], dtype=np.uint64), data)
    if l1_tile is not None:
        idx.set_option("l1_tile", l1_tile)
    return idx


# ---------------------------------------------------------------------------
# provider
# ---------------------------------------------------------------------------
def test_provider_known_answers(wv):
    """manhattan_test.go:21-65"""
    for a, b, want in [((3, 4, 5), (3, 4, 5), 0.0), ((3, 4, 5), (1.5, 2, 2.5), 6.0), ((10, 11), (13, 15), 7.0)]:
        got = wv.single_dist_batch("manhattan", np.array(a, np.float32), np.array(b, np.float32))
        assert got.shape == (1,) and got[0] == np.float32(want)


@pytest.mark.parametrize("d", [1, 3, 8, 13, 45, 128, 200, 769])
def test_provider_equals_sequential_sum(wv, d):
    a, b = uniform(100 + d, 64, d), uniform(200 + d, 64, d)
    got = wv.single_dist_batch("manhattan", a, b)
    np.testing.assert_array_equal(got.view(np.uint32), l1(a, b).view(np.uint32))


def test_provider_length_mismatch(wv):
    with pytest.raises(wv.WeaviateError, match="3 vs 2: vector lengths don't match"):
        wv.single_dist_batch("manhattan", np.zeros(3, np.float32), np.zeros(2, np.float32))


def test_order_sensitivity(wv):
    """The fixture discriminates: a pairwise (or any other) summation order
    differs from the sequential one on these pairs, so only a kernel that sums
    in element order passes -- the provider and both search kernels."""
    d, n = 200, 512
    a, b = uniform(7, n, d), uniform(8, n, d)
    seq = l1(a, b)
    pairwise = np.sum(np.abs(a - b), axis=-1, dtype=np.float32)
    assert np.count_nonzero(seq.view(np.uint32) != pairwise.view(np.uint32)) >= 1
    got = wv.single_dist_batch("manhattan", a, b)
    np.testing.assert_array_equal(got.view(np.uint32), seq.view(np.uint32))
    # rows b against the one query a[0], every distance returned (k = n), through both kernels
    want = np.sort(l1(a[0], b))
    for tile in (0, 1):
        idx = make_index(wv, b, tile)
        _, gd, gn = idx.search_by_vector_batch(a[:1], n)
        idx.close()
        assert gn[0] == n
        np.testing.assert_array_equal(gd[0].view(np.uint32), want.view(np.uint32), err_msg=f"l1_tile={tile}")


# ---------------------------------------------------------------------------
# search, both kernels
# ---------------------------------------------------------------------------
SEARCH_CASES = [  # n, d, nq, k
    (1, 1, 1, 10),       # one row, k > n
    (255, 200, 12, 1),
    (255, 3, 7, 10),
    (256, 128, 12, 100),
    (257, 45, 33, 10),   # a second row block of one row, ragged last query tile, a 1-element tail
    (3000, 200, 33, 100),
    (3000, 128, 1, 10),
    (3000, 1, 7, 10),
]


@pytest.mark.parametrize("l1_tile", [0, 1])
@pytest.mark.parametrize("n,d,nq,k", SEARCH_CASES)
def test_search_equals_reference_heap(wv, oracle, l1_tile, n, d, nq, k):
    data, queries = uniform(11 * n + d, n, d), uniform(13 * n + d, nq, d)
    idx = make_index(wv, data, l1_tile)
    got = idx.search_by_vector_batch(queries, k)
    route = idx.stats()["last_route"]
    idx.close()
    assert (route == ROUTE_L1_TILE) == (l1_tile == 1)
    check_batch(oracle, got, data, np.arange(n), queries, k, f"l1_tile={l1_tile}")


def test_auto_route_by_list_length(wv, oracle):
    """Option l1_tile = -1 (the default): one query takes the lane-per-pair
    kernel, two or more the tiled one (profiles/l1_tile_ab.json)."""
    n, d, k = 700, 45, 10
    data, queries = uniform(15, n, d), uniform(16, 2, d)
    idx = make_index(wv, data)
    one = idx.search_by_vector_batch(queries[:1], k)
    r1 = idx.stats()["last_route"]
    two = idx.search_by_vector_batch(queries, k)
    r2 = idx.stats()["last_route"]
    idx.close()
    assert r1 != ROUTE_L1_TILE and r2 == ROUTE_L1_TILE
    check_batch(oracle, one, data, np.arange(n), queries[:1], k, "one query")
    check_batch(oracle, two, data, np.arange(n), queries, k, "two queries")


@pytest.mark.parametrize("l1_tile", [0, 1])
def test_wide_rows_cross_the_query_chunk(wv, oracle, l1_tile):
    """d above 512: k_l1_rows stages the queries in more than one LDS chunk; the
    accumulators carry over the chunk boundary (d = 1100: chunks of 512, 512, 76)."""
    n, d, nq, k = 300, 1100, 9, 10
    data, queries = uniform(21, n, d), uniform(22, nq, d)
    idx = make_index(wv, data, l1_tile)
    got = idx.search_by_vector_batch(queries, k)
    idx.close()
    check_batch(oracle, got, data, np.arange(n), queries, k, f"l1_tile={l1_tile}")


@pytest.mark.parametrize("l1_tile", [0, 1])
@pytest.mark.parametrize("k", [10, 100])
def test_ties_follow_the_reference_heap(wv, oracle, l1_tile, k):
    """Integer data U{0..3}, d = 8: distances in 0..24, every k-th boundary tied."""
    n, d, nq = 3000, 8, 12
    rng = np.random.default_rng(31)
    data = rng.integers(0, 4, size=(n, d)).astype(np.float32)
    queries = rng.integers(0, 4, size=(nq, d)).astype(np.float32)
    idx = make_index(wv, data, l1_tile)
    got = idx.search_by_vector_batch(queries, k)
    idx.close()
    check_batch(oracle, got, data, np.arange(n), queries, k, f"l1_tile={l1_tile}")


# ---------------------------------------------------------------------------
# writes and filters
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("l1_tile", [0, 1])
def test_writes_and_filters(wv, oracle, l1_tile):
    n, d, nq, k = 3000, 45, 12, 10
    data, queries = uniform(41, n, d), uniform(42, nq, d)
    idx = make_index(wv, data, l1_tile)
    rng = np.random.default_rng(43)
    dele = rng.choice(n, n // 10, replace=False)
    idx.delete(*[int(x) for x in np.sort(dele)])
    ups = np.sort(rng.choice(n, 50, replace=False))  # deleted and live ids alike, new values
    data = data.copy()
    data[ups] = uniform(44, len(ups), d)
    idx.add_batch(ups.astype(np.uint64), data[ups])
    present = np.ones(n, bool)
    present[dele] = False
    present[ups] = True
    pid = np.flatnonzero(present)
    check_batch(oracle, idx.search_by_vector_batch(queries, k), data[pid], pid, queries, k, "after writes")

    allowed = np.sort(rng.choice(n, 400, replace=False))
    aid = allowed[present[allowed]]
    got = idx.search_by_vector_batch(queries, k, allow=wv.AllowList(allowed))
    check_batch(oracle, got, data[aid], aid, queries, k, "allow list")
    _, _, cnt = idx.search_by_vector_batch(queries, k, allow=wv.AllowList([]))
    assert not cnt.any()

    # SearchByVectorDistance: k = 100, then the prefix within the target (+ 1e-6)
    q = queries[0]
    ei, ed = expect(oracle, data[pid], pid, q, 100)
    target = float(ed[39])
    keep = [j for j in range(len(ed)) if ed[j] <= target or abs(float(ed[j]) - target) <= 1e-6]
    gi, gd = idx.search_by_vector_distance(q, target, 10000)
    assert 40 <= len(gi) == len(keep) <= 45
    np.testing.assert_array_equal(gi, ei[keep])
    np.testing.assert_array_equal(gd.view(np.uint32), ed[keep].view(np.uint32))

    # the single-query entry (micro-batcher)
    gi, gd = idx.search_by_vector(queries[1], k)
    ei, ed = expect(oracle, data[pid], pid, queries[1], k)
    np.testing.assert_array_equal(gi, ei)
    np.testing.assert_array_equal(gd.view(np.uint32), ed.view(np.uint32))

    # QueryVectorDistancer
    some = pid[:: max(1, len(pid) // 37)]
    gd = idx.query_vector_distances(queries[2], some)
    np.testing.assert_array_equal(gd.view(np.uint32), l1(queries[2], data[some]).view(np.uint32))
    idx.close()


# ---------------------------------------------------------------------------
# non-finite
# ---------------------------------------------------------------------------
def _nonfinite_fixture(nan):
    n, d, nq = 600, 13, 12
    data, queries = uniform(51, n, d), uniform(52, nq, d)
    rng = np.random.default_rng(53)
    rows = rng.choice(n, 60, replace=False)
    data[rows[:30], 2] = np.inf
    data[rows[30:], 2] = -np.inf
    queries[3, 5] = np.inf   # every distance of these two queries is +inf
    queries[7, 5] = -np.inf
    if nan:
        data[rng.choice(n, 40, replace=False), 7] = np.nan
        queries[9, 2] = np.inf   # inf - inf against the rows above
        queries[10, 11] = np.nan  # every distance NaN
    return data, queries


def _both_kernels(wv, data, queries, k):
    out = []
    for tile in (0, 1):
        idx = make_index(wv, data, tile)
        out.append(idx.search_by_vector_batch(queries, k))
        idx.close()
    (i0, d0, n0), (i1, d1, n1) = out
    np.testing.assert_array_equal(n0, n1)
    np.testing.assert_array_equal(i0, i1)
    np.testing.assert_array_equal(d0, d1)  # NaN == NaN
    np.testing.assert_array_equal(np.isnan(d0), np.isnan(d1))
    return out[1]


@pytest.mark.parametrize("k", [10, 100])
def test_infinite_elements(wv, oracle, k):
    data, queries = _nonfinite_fixture(nan=False)
    assert not np.isnan(l1(queries[:, None, :], data[None])).any()
    got = _both_kernels(wv, data, queries, k)
    check_batch(oracle, got, data, np.arange(len(data)), queries, k, "inf")


@pytest.mark.parametrize("k", [10, 100])
def test_nan_distances(wv, oracle, k):
    """NaN distances (NaN elements, inf - inf): both kernels agree bitwise, and
    the replay equals the reference heap, NaN compared as NaN == NaN."""
    data, queries = _nonfinite_fixture(nan=True)
    assert np.isnan(l1(queries[:, None, :], data[None])).any()
    got = _both_kernels(wv, data, queries, k)
    check_batch(oracle, got, data, np.arange(len(data)), queries, k, "nan", nan_ok=True)


# ---------------------------------------------------------------------------
# BQ + manhattan
# ---------------------------------------------------------------------------
def bq_expect(oracle, data, codes, q, k, rescore_limit):
    """searchByVectorQuantized: the R-heap over bitwise hamming of the sign
    codes, popped max-first, each candidate rescored with the provider and
    offered to the k-heap in pop order."""
    R = max(rescore_limit, k)
    qc = oracle.bq_encode(q)
    ham = np.array([oracle.hamming_bitwise(c, qc) for c in codes], np.float32)
    cand, _ = oracle.heap_scan(ham, R)
    pop = cand[::-1].astype(np.int64)
    pos, dd = oracle.heap_scan(l1(q, data[pop]), k)
    return pop[pos.astype(np.int64)].astype(np.uint64), dd


@pytest.mark.parametrize("rescore_limit", [-1, 50])
def test_bq_rescoring_uses_the_provider(wv, oracle, rescore_limit):
    n, d, nq, k = 3000, 128, 6, 10
    data, queries = uniform(61, n, d), uniform(62, nq, d)
    codes = [oracle.bq_encode(r) for r in data]
    idx = make_index(wv, data, bq=True, rescore_limit=rescore_limit)
    gi, gd, gn = idx.search_by_vector_batch(queries, k)
    idx.close()
    for i, q in enumerate(queries):
        ei, ed = bq_expect(oracle, data, codes, q, k, rescore_limit)
        assert gn[i] == len(ei) == k
        np.testing.assert_array_equal(gi[i], ei, err_msg=f"q{i} ids")
        np.testing.assert_array_equal(gd[i].view(np.uint32), ed.view(np.uint32), err_msg=f"q{i} dists")


# ---------------------------------------------------------------------------
# multi-shard
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("bq", [False, True])
def test_multi_equals_single(wv, oracle, bq):
    """3 shards on device 0, local transport: exact goes through the shard
    fallback (phase 1 unsupported -> search_device mode 1, merge, replay), BQ
    through the BQ protocol."""
    from weaviate_amd.multi import MultiFlatIndex
    n, d, nq, k, shards = 3000, 45, 33, 10, 3
    data, queries = uniform(71, n, d), uniform(72, nq, d)
    single = make_index(wv, data, bq=bq)
    want = single.search_by_vector_batch(queries, k)
    single.close()
    m = MultiFlatIndex(distance="manhattan", dims=d, devices=[0] * shards, id_stride=n // shards, transport="local",
                       variant="avx256", bq=bq)
    m.add_batch(np.arange(n, dtype=np.uint64), data)
    got = m.search_by_vector_batch(queries, k)
    m.close()
    np.testing.assert_array_equal(got[2], want[2])
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(got[1].view(np.uint32), want[1].view(np.uint32))
    if not bq:
        check_batch(oracle, got, data, np.arange(n), queries, k, "multi")
