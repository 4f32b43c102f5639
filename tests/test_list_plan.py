"""The host planner of the list-order hnsw flat search
(weaviate_amd/csrc/list_plan.h): tools/list_plan_print.cpp compiled against the
header alone, its plans for two hand-written batches compared with values
worked out by hand below -- the pool (ascending, distinct, in-range slots,
identical lists stored once), the per-query ranges, the work table and the
launch groups.  The same program is also built with the address and undefined
behaviour sanitizers and run on the same batches (stand-alone host code)."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tools", "list_plan_print.cpp")

# batch A: id_base 100, hiwater 1000 (ids 100 .. 1099 are in range), budget 1024 entries, 2 chunks per piece
A_IN = (100, 1000, 1024, 2, [
    (0, []),                                    # row 0: no list, not part of the plan
    (1, []),                                    # row 1: the empty list
    (1, [1100, 5000, 99, 3]),                   # row 2: only out-of-range ids (1100 = id_base + hiwater), unsorted
    (1, [105, 50, 103, 105, 99, 103, 101]),     # row 3: duplicates, unsorted, ids below id_base -> slots 1 3 5
    (1, [100, 101, 150, 1099, 1100]),           # row 4: ascending (the no-sort path) -> slots 0 1 50 999
    (1, [101, 103, 105]),                       # row 5: row 3's normalised content -> shares its storage
    (2, 4),                                     # row 6: row 4's caller range again -> shares its storage
])
A_OUT = {
    "pool": [1, 3, 5, 0, 1, 50, 999],
    # (batch row, pool begin, length, first entry in the group's buffers)
    "q": [(1, 0, 0, 0), (2, 0, 0, 0), (3, 0, 3, 0), (4, 3, 4, 256), (5, 0, 3, 512), (6, 3, 4, 768)],
    # (listed query, first entry, count)
    "p": [(2, 0, 3), (3, 0, 4), (4, 0, 3), (5, 0, 4)],
    # (listed queries [lq0, lq1), pieces [p0, p1), entries): 4 lists of one chunk fill the budget exactly
    "g": [(0, 6, 0, 4, 1024)],
    # scanned 3 + 4 + 3 + 4, sorted: rows 2 and 3, shared: rows 2 (empty like row 1), 5, 6, largest group
    "s": (14, 2, 3, 1024),
}

# batch B: chunk edges (255 / 256 / 257 entries), a budget of 600 entries that
# splits the batch, and a list of 1500 entries that is longer than the budget
B_IN = (0, 100000, 600, 2, [
    (1, list(range(0, 255))),
    (1, list(range(1000, 1256))),
    (1, list(range(2000, 2257))),
    (1, list(range(0, 1500))),
    (1, [7]),
])
B_OUT = {
    "pool": list(range(0, 255)) + list(range(1000, 1256)) + list(range(2000, 2257)) + list(range(0, 1500)) + [7],
    # padded entries 256, 256, 512, 1536, 256: rows 0 + 1 make 512; row 2 would pass 600 and opens a group, and so on
    "q": [(0, 0, 255, 0), (1, 255, 256, 256), (2, 511, 257, 0), (3, 768, 1500, 0), (4, 2268, 1, 0)],
    # 2 chunks = 512 entries per piece: 1500 = 512 + 512 + 476
    "p": [(0, 0, 255), (1, 0, 256), (2, 0, 257), (3, 0, 512), (3, 512, 512), (3, 1024, 476), (4, 0, 1)],
    "g": [(0, 2, 0, 2, 512), (2, 3, 2, 3, 512), (3, 4, 3, 6, 1536), (4, 5, 6, 7, 256)],
    "s": (2269, 0, 0, 1536),
}


def _text(batch):
    id_base, hiwater, budget, cpw, rows = batch
    lines = [f"{id_base} {hiwater} {budget} {cpw} {len(rows)}"]
    for mode, v in rows:
        lines.append(f"2 {v}" if mode == 2 else f"{mode} {len(v)} " + " ".join(str(x) for x in v))
    return "\n".join(lines) + "\n"


def _parse(out):
    got = {"pool": None, "q": [], "p": [], "g": [], "s": None}
    for line in out.split("\n"):
        w = line.split()
        if not w:
            continue
        v = [int(x) for x in w[1:]]
        if w[0] == "pool":
            got["pool"] = v
        elif w[0] == "s":
            got["s"] = tuple(v)
        else:
            got[w[0]].append(tuple(v))
    return got


def _check(exe, env=None):
    for batch, want in ((A_IN, A_OUT), (B_IN, B_OUT)):
        r = subprocess.run([exe], input=_text(batch), capture_output=True, text=True, env=env)
        assert r.returncode == 0, r.stderr
        got = _parse(r.stdout)
        for key in ("pool", "q", "p", "g", "s"):
            assert got[key] == want[key], f"{key}: {got[key]} expected {want[key]}"
        # the properties every plan has, whatever the table says
        for row, begin, n, e_begin in got["q"]:
            sl = got["pool"][begin:begin + n]
            assert all(a < b for a, b in zip(sl, sl[1:])) and all(0 <= s < batch[1] for s in sl)
            assert e_begin % 256 == 0
        assert all(lq1 > lq0 for lq0, lq1, _, _, _ in got["g"])


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_list_plan_table(tmp_path):
    exe = str(tmp_path / "list_plan_print")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", SRC, "-o", exe], check=True)
    _check(exe)


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_list_plan_table_sanitized(tmp_path):
    exe = str(tmp_path / "list_plan_print_san")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", SRC,
                        "-o", exe], capture_output=True, text=True)
    if r.returncode != 0:
        pytest.skip("g++ cannot link the sanitizer runtimes here")
    _check(exe, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
