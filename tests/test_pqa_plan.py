"""The host planner of a multi-allow batch (weaviate_amd/csrc/pqa_plan.h):
tools/pqa_plan_print.cpp compiled against the header alone, its plans for
hand-written batches compared with steps worked out by hand below -- who shares
a launch, with which select depths m and list size R, who is searched grouped
by list, where the bitmap budget cuts and when a bitmap form goes through id
lists.  The same program is also built with the address and undefined
behaviour sanitizers and run on the same batches (stand-alone host code)."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tools", "pqa_plan_print.cpp")

U = (0, 0)  # an unlisted row


def L(size):
    return (1, size)


def case(rows, k=10, npresent=100000, qmax_ids=1000, qmax_bits=0, split_max=64, shared=1, keyed=1, own_keys=0,
         quant_max=-1):
    return dict(rows=rows, k=k, npresent=npresent, qmax_ids=qmax_ids, qmax_bits=qmax_bits, split_max=split_max,
                shared=shared, keyed=keyed, own_keys=own_keys, quant_max=quant_max)


def launch(R, rows, m):
    return ("l", R, list(rows), list(m))


def grouped(rows):
    return ("g", list(rows))


# k = 10 throughout: an unlisted row's depth is k + 1 = 11, a listed row's 22 max(1, U / size)
A_ROWS = [U, L(50000), L(1000), L(20)]
CASES = {
    # A: tot = 100000 + 50000 + 1000 + 20 -> U = npresent = 100000; depths 11, 22 * 2 = 44, 22 * 100 = 2200,
    # 22 * 5000 = 110000: rows 2 and 3 are deeper than 960 and leave; rows 0, 1 retaken (U stays 100000): 11, 44
    "A": (case(A_ROWS), 0, [grouped([2, 3]), launch(8, [0, 1], [11, 44])]),
    # A': two sparse rows > split_max = 1: no split; m clamps at 960, above 448 -> R = 16
    "A1": (case(A_ROWS, split_max=1), 0, [launch(16, [0, 1, 2, 3], [11, 44, 960, 960])]),
    # A'': per-query keys serve sparse lists in the launch
    "A2": (case(A_ROWS, own_keys=1), 0, [launch(16, [0, 1, 2, 3], [11, 44, 960, 960])]),
    # B: tot = U = 2020: 22 * 2.02 = 44.44, 44.44, 22 * 101 = 2222 -> row 2 leaves; the launched batch has
    # tot = U = 2000: 22 * 2 = 44 exactly (45 = ceil(44.44) would be the caller's batch's tot)
    "B": (case([L(1000), L(1000), L(20)]), 0, [grouped([2]), launch(8, [0, 1], [44, 44])]),
    # C: tot = U = 51020: 22 * 1.02 = 22.4, 22 * 51.02 = 1122, 22 * 2551 = 56122 -> rows 1, 2 leave, and the
    # dense half is one row: no launch
    "C": (case([L(50000), L(1000), L(20)]), 0, [grouped([1, 2]), grouped([0])]),
    # D: runs of qmax_ids = 2; the last run is one row
    "D": (case([U] * 5, qmax_ids=2), 0, [launch(8, [0, 1], [11, 11]), launch(8, [2, 3], [11, 11]), grouped([4])]),
    # D': the caller's batch: tot = 103020 -> U = 100000: rows 0-2 22 * 100 = 2200, rows 3, 4 44, row 5 110000:
    # four rows deeper than 960 > split_max = 1, no split.  Runs of 3: rows 0-2 have tot = U = 3000 ->
    # 22 * 3 = 66, nothing to split; rows 3-5 have tot = 100020 -> U = 100000: 44, 44, 110000 -> row 5 leaves
    # (1 <= split_max), rows 3, 4 retaken with tot = U = 100000: 44, 44
    "D1": (case([L(1000), L(1000), L(1000), L(50000), L(50000), L(20)], qmax_ids=3, split_max=1), 0,
           [launch(8, [0, 1, 2], [66, 66, 66]), grouped([5]), launch(8, [3, 4], [44, 44])]),
    # E: 3 rows > qmax_bits = 2: the id-list form's plan (3 <= qmax_ids = 4: one launch)
    "E": (case([U] * 3, qmax_ids=4, qmax_bits=2), 1, [launch(8, [0, 1, 2], [11, 11, 11])]),
    "E1": (case([U] * 3, qmax_ids=4, qmax_bits=4), 0, [launch(8, [0, 1, 2], [11, 11, 11])]),
    # E'': A as bitmaps within the budget: it would split, so A's plan through lists
    "E2": (case(A_ROWS, qmax_bits=500), 1, [grouped([2, 3]), launch(8, [0, 1], [11, 44])]),
    # F: a quantized route: no depths (m = 0, R = 8), no split (rows 1, 2 stay), round_up(n, 256) <= quant_max
    "F200": (case([U, L(20), L(5)] + [L(50000)] * 197, keyed=0, quant_max=256), 0,
             [launch(8, range(200), [0] * 200)]),
    "F300": (case([U] * 300, keyed=0, quant_max=256), 0, [grouped(range(300))]),  # round_up(300, 256) = 512
    "F1": (case([U], keyed=0, quant_max=256), 0, [grouped([0])]),
    # the one-chunk rule sees the sub-batches' size: min(300, 256) = 256 fits, runs of 256 and 44
    "F300cut": (case([U] * 300, keyed=0, quant_max=256, qmax_ids=256), 0,
                [launch(8, range(256), [0] * 256), launch(8, range(256, 300), [0] * 44)]),
    # BQ: no limit
    "Fbq": (case([U] * 300, keyed=0), 0, [launch(8, range(300), [0] * 300)]),
    # G: nothing shares a launch (as a bitmap form: lists for everybody)
    "G": (case(A_ROWS, shared=0), 0, [grouped([0, 1, 2, 3])]),
    "Gbits": (case(A_ROWS, shared=0, qmax_bits=500), 1, [grouped([0, 1, 2, 3])]),
    "empty": (case([]), 0, []),
}


def _text(c):
    head = [len(c["rows"]), c["k"], c["npresent"], c["qmax_ids"], c["qmax_bits"], c["split_max"], c["shared"],
            c["keyed"], c["own_keys"], c["quant_max"]]
    return " ".join(str(x) for x in head) + "\n" + "".join(f"{m} {s}\n" for m, s in c["rows"])


def _parse(out):
    via, steps = None, []
    for line in out.split("\n"):
        w = line.split()
        if not w:
            continue
        v = [int(x) for x in w[1:]]
        if w[0] == "v":
            via = v[0]
        elif w[0] == "l":
            n = v[1]
            assert len(v) == 2 + 2 * n, "m has one entry per row of its step"
            steps.append(("l", v[0], v[2:2 + n], v[2 + n:]))
        else:
            assert w[0] == "g" and len(v) == 1 + v[0]
            steps.append(("g", v[1:]))
    return via, steps


def _check(exe, env=None):
    for name, (c, want_via, want) in CASES.items():
        r = subprocess.run([exe], input=_text(c), capture_output=True, text=True, env=env)
        assert r.returncode == 0, (name, r.stderr)
        via, steps = _parse(r.stdout)
        assert via == want_via, name
        assert steps == want, f"{name}: {steps} expected {want}"
        # the properties every plan has, whatever the table says
        seen = sorted(q for st in steps for q in st[-1 if st[0] == "g" else 2])
        assert seen == list(range(len(c["rows"]))), f"{name}: every row in exactly one step"
        for st in steps:
            if st[0] == "l":
                assert 2 <= len(st[2]) <= c["qmax_ids"], name
                assert via or not c["qmax_bits"] or len(st[2]) <= c["qmax_bits"], name
                assert len(st[3]) == len(st[2]), name


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_pqa_plan_table(tmp_path):
    exe = str(tmp_path / "pqa_plan_print")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", SRC, "-o", exe], check=True)
    _check(exe)


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_pqa_plan_table_sanitized(tmp_path):
    exe = str(tmp_path / "pqa_plan_print_san")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", SRC,
                        "-o", exe], capture_output=True, text=True)
    if r.returncode != 0:
        pytest.skip("g++ cannot link the sanitizer runtimes here")
    _check(exe, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
