"""CPU: the manhattan distance through the host-only layers -- the config
validation texts, the compression matrix refused at create (before any device
call) and the public header's two new defines."""
import ctypes as C
import os
import re

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_distance_is_immutable_text(wv):
    from weaviate_amd.flat import validate_user_config_update as v
    v(dict(distance="manhattan"), dict(distance="manhattan"))
    with pytest.raises(wv.WeaviateError,
                       match='distance is immutable: attempted change from "manhattan" to "l2-squared"'):
        v(dict(distance="manhattan"), dict(distance="l2-squared"))
    with pytest.raises(wv.WeaviateError,
                       match='distance is immutable: attempted change from "hamming" to "manhattan"'):
        v(dict(distance="hamming"), dict(distance="manhattan"))


def _create(cfg):
    from weaviate_amd import _lib
    lib = _lib.load()
    h = C.c_void_p()
    rc = lib.wv_index_create(C.byref(cfg), C.byref(h))
    msg = (lib.wv_last_error() or b"").decode()
    if rc == 0:  # not expected in these cases; never leak a handle
        lib.wv_index_destroy(h)
    return rc, msg


@pytest.mark.parametrize("kw", [dict(rq={"bits": 8}), dict(rq={"bits": 1}), dict(sq=True)])
def test_rq_and_sq_refuse_manhattan_at_create(wv, kw):
    """rotational_quantization.go:41-45 and scalar_quantization.go:49-57 have no
    manhattan arm; the refusal comes before the first device call (no GPU here)."""
    from weaviate_amd import _lib
    from weaviate_amd.flat import make_config
    rc, msg = _create(make_config(distance="manhattan", dims=16, **kw))
    assert rc == _lib.WV_ERR_UNSUPPORTED
    assert msg == "Distance not supported yet manhattan"


def test_pq_refuses_manhattan_at_create(wv):
    from weaviate_amd import _lib
    from weaviate_amd.flat import make_config
    rc, msg = _create(make_config(distance="manhattan", dims=16, pq={"segments": 4}))
    assert rc == _lib.WV_ERR_UNSUPPORTED
    assert "manhattan" in msg


def test_flat_index_raises_the_reference_text(wv):
    with pytest.raises(wv.WeaviateError, match="Distance not supported yet manhattan") as e:
        wv.FlatIndex(distance="manhattan", dims=16, rq={"bits": 8})
    assert e.value.code == -5


def test_header_declares_metric_and_route():
    src = open(os.path.join(REPO, "include", "wv_knn.h")).read()
    defs = dict(re.findall(r"^#define\s+(WV_[A-Z0-9_]+)\s+(-?\d+)\b", src, flags=re.M))
    assert defs["WV_METRIC_MANHATTAN"] == "4"
    assert defs["WV_ROUTE_L1_TILE"] == "11"
    # no two metrics and no two routes share a value
    for prefix in ("WV_METRIC_", "WV_ROUTE_"):
        vals = [v for k, v in defs.items() if k.startswith(prefix)]
        assert len(vals) == len(set(vals))
    from weaviate_amd import _lib
    from weaviate_amd.flat import DISTANCES, PROVIDER_TYPE
    assert _lib.METRIC_MANHATTAN == 4 and DISTANCES["manhattan"] == 4 and PROVIDER_TYPE[4] == "manhattan"
    assert _lib.ROUTES[11] == "l1_tile"
