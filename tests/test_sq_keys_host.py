"""The SQ integer-MFMA route's public names (no GPU): the route constant of the
header and its name in the Python table."""
import os
import re

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_route_14_is_sq_int8():
    from weaviate_amd import _lib
    src = open(os.path.join(REPO, "include", "wv_knn.h")).read()
    defs = dict(re.findall(r"^#define\s+(WV_ROUTE_[A-Z0-9_]+)\s+(\d+)\b", src, flags=re.M))
    assert defs["WV_ROUTE_SQ_INT8"] == "14"
    assert _lib.ROUTES[14] == "sq_int8"
    assert sorted(int(v) for v in defs.values()) == sorted(_lib.ROUTES)  # every route has a name, none twice
