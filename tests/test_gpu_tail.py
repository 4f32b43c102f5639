"""GPU parity of the block-key search's tail after the int8 key pass
(DESIGN.md §3.1h): k_blk_select_f's 16-byte key loads, the one-wave-per-block
int8 row filter k_q8_filt_bm and k_blk_exact's short top lists under a finite
cap.  Ids, distances and counts bit-exact against the oracle, and the
per-query filter arm (q8_bm 0) bit-equal to the block-major default.

Every index here sets sel_split_max = 0: batches of up to 512 queries take the
split selection (k_sel_*) by default and would never launch k_blk_select_f.

Shapes: 96 queries (above q8_bm_min, no multiple of 64), a last block partly
past the high-water mark.  At d = 768 the rows are wider than 508 floats: the
block-major filter and the short lists (cosine, l2-squared; dot in the last
test).  l2-squared at d = 400 has rows of 400 floats and takes k_exact_bm
instead: the read-back exact kernel, which keeps the full list depth.  The key row holds nb = 2 ceil(rows / 64) keys:
  20,037 rows  nb =  628: one ragged chunk (the permuted scalar loads of an
               aligned row), every filter workgroup full;
  40,037 rows  nb = 1252: an aligned row, one full float4 chunk of 1024 keys,
               then the ragged chunk;
  40,100 rows  nb = 1254: rows that are not 16-byte aligned (scalar loads on
               full chunks), a last filter workgroup with two idle waves.
Each test reads nb back from the library and asserts these properties; the
two longer shapes also search 94 queries (a select workgroup with two idle
waves)."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_flat import assert_same, build_pair, gen

pytestmark = pytest.mark.gpu

ROUTE_INT8 = 3
# the filtering select (k_blk_select_f) at every batch size instead of the split selection
FILTERING_SELECT = {"sel_split_max": 0}
N, B, NDUP, NDEL, NTIE = 20037, 96, 40, 300, 12


def list_depth_ks(wv):
    """k = 10, the largest k with k = 10's list depth, and the first k past it
    (qs_R_flat, the library's own table)."""
    # int qs_R_flat(int) (qs_runtime.hip) has no C name and this change may add none: its C++ symbol
    fn = getattr(wv.load(), "_Z9qs_R_flati", None)
    assert fn is not None, "libwvknn.so no longer exports int qs_R_flat(int) as _Z9qs_R_flati: update this lookup"
    fn.restype, fn.argtypes = C.c_int, [C.c_int]
    kb = 10
    while fn(kb + 1) == fn(10):
        kb += 1
    assert 10 < kb < 200
    return [10, kb, kb + 1]


_cases = {}


@pytest.fixture(scope="module", autouse=True)
def close_cases():
    yield
    for idx, _, _, _ in _cases.values():
        idx.close()
    _cases.clear()


def tail_case(wv, oracle, metric, d, N=N):
    """Index, oracle and queries of one shape, built once: 40 rows duplicate
    another row exactly, 300 rows are deleted, the first 12 queries are
    duplicated rows (their two nearest rows tie: no strict top-(k+1), the
    replay decides), the others are independent."""
    if (metric, d, N) not in _cases:
        rng = np.random.default_rng(91)
        data = gen(oracle, 0, 92, N, d)
        src = rng.choice(N // 2, NDUP, replace=False)
        dst = N // 2 + rng.choice(N // 2, NDUP, replace=False)
        data[dst] = data[src]
        idx, orc = build_pair(wv, oracle, metric, "avx256", data, options=FILTERING_SELECT)
        dele = np.setdiff1d(rng.choice(N, NDEL, replace=False), np.concatenate([src, dst]))
        idx.delete(*[int(x) for x in dele])
        orc.delete([int(x) for x in dele])
        queries = gen(oracle, 0, 93, B, d)
        queries[:NTIE] = data[src[:NTIE]]
        _cases[(metric, d, N)] = (idx, orc, queries, {})
    return _cases[(metric, d, N)]


def reference(case, k):
    _, orc, queries, refs = case
    if k not in refs:
        refs[k] = [orc.search(q, k) for q in queries]
    return refs[k]


def run(idx, queries, k):
    before = idx.stats()["replayed_queries"]
    got = idx.search_by_vector_batch(queries, k)
    assert idx.stats()["last_route"] == ROUTE_INT8
    return got, idx.stats()["replayed_queries"] - before


def key_row_length(idx):
    """nb of the last block-key batch: the select's key row and the filter's block count"""
    return len(idx.debug_blockkeys(0)[0])


def check_arms(case, k):
    """Default (block-major filter) against the oracle, the per-query filter bit-equal to it;
    -> replayed queries."""
    idx, _, queries, _ = case
    ref = reference(case, k)
    (ids, dists, counts), replayed = run(idx, queries, k)
    for qi in range(B):
        assert_same(ref[qi], ids[qi, :counts[qi]], dists[qi, :counts[qi]], ctx=f"k{k} q{qi}")
    idx.set_option("q8_bm", 0)  # the per-query filter: the short lists without masks
    try:
        (ids0, dists0, counts0), replayed0 = run(idx, queries, k)
    finally:
        idx.set_option("q8_bm", 1)
    assert replayed0 == replayed
    np.testing.assert_array_equal(counts0, counts)
    np.testing.assert_array_equal(ids0, ids)
    np.testing.assert_array_equal(dists0.view(np.uint32), dists.view(np.uint32))
    return replayed


@pytest.mark.parametrize("ki", [0, 1, 2])
@pytest.mark.parametrize("metric,d", [("cosine", 768), ("l2-squared", 400), ("l2-squared", 768)])
def test_tail_matches_oracle_and_per_query_filter(wv, oracle, metric, d, ki):
    k = list_depth_ks(wv)[ki]
    case = tail_case(wv, oracle, metric, d)
    idx, orc, queries, _ = case
    # the seed's ties: some queries have equal distances among their k+1 nearest, not all
    tied = [bool((np.diff(orc.search(q, k + 1)[2]) == 0).any()) for q in queries]
    assert any(tied) and not all(tied)
    replayed = check_arms(case, k)
    print(f"{metric} d={d} k={k}: {sum(tied)} tied queries, {replayed} replayed")
    assert 1 <= replayed < B
    nb = key_row_length(idx)
    assert nb < 1024 and nb % 4 == 0  # the ragged chunk of an aligned row


@pytest.mark.parametrize("n,aligned", [(40037, True), (40100, False)])
def test_tail_key_rows_past_one_chunk(wv, oracle, n, aligned):
    """Key rows longer than one 1024-key chunk and no multiple of it: a 16-byte
    aligned row (a full float4 chunk, then the ragged one) and an unaligned one
    (scalar loads on full chunks; nb % 4 = 2: two idle waves in the filter's
    last workgroup)."""
    case = tail_case(wv, oracle, "cosine", 768, N=n)
    replayed = check_arms(case, 10)
    assert 1 <= replayed < B
    idx, _, queries, _ = case
    nb = key_row_length(idx)
    assert nb > 1024 and nb % 1024 != 0
    assert (nb % 4 == 0) == aligned and (aligned or nb % 4 == 2)
    # four queries per select workgroup: 94 leave the last one two idle waves
    (ids, dists, counts), _ = run(idx, queries[:B - 2], 10)
    ref = reference(case, 10)
    for qi in range(B - 2):
        assert_same(ref[qi], ids[qi, :counts[qi]], dists[qi, :counts[qi]], ctx=f"94 queries q{qi}")


def test_tail_dot_with_one_huge_row(wv, oracle):
    """dot with one row of 1000 times the norm: every query's bound overflows
    or flags there; the results still equal the oracle's."""
    d, k = 768, 10
    data = gen(oracle, 0, 94, N, d)
    data[N // 3] *= np.float32(1000.0)
    queries = gen(oracle, 0, 95, B, d)
    idx, orc = build_pair(wv, oracle, "dot", "avx256", data, options=FILTERING_SELECT)
    try:
        ids, dists, counts = idx.search_by_vector_batch(queries, k)
        assert idx.stats()["last_route"] == ROUTE_INT8
        for qi in range(B):
            assert_same(orc.search(queries[qi], k), ids[qi, :counts[qi]], dists[qi, :counts[qi]], ctx=f"q{qi}")
    finally:
        idx.close()
