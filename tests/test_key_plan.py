"""The span planner of the block-key passes (weaviate_amd/csrc/key_plan.h) on
the host: tools/key_plan_print.cpp compiled against the header, its plans
compared with values worked out from the three hand-written copies of the
arithmetic the header replaced.  The rows where the 4 GiB buffer-offset bound
binds (10^8 slots, 6144-byte rows, 3 * 10^7 slots with a `spans` option) are
out of any GPU test's reach: this is their only check."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# nqg, nslots, RB, row bytes, `spans` option, whole rounds -> slots per span, nspans
TABLE = [
    (1, 1, 2, 768, 0, True, 1, 1),
    (1, 5, 2, 768, 0, True, 1, 5),
    (1, 1000, 2, 768, 0, True, 4, 250),
    (32, 156250, 2, 768, 0, True, 19532, 8),
    (3, 156250, 2, 768, 0, True, 611, 256),
    (5, 9766, 1, 1536, 0, True, 39, 251),
    (32, 39063, 2, 768, 7, True, 5581, 7),
    (1, 40, 2, 768, 1, True, 40, 1),
    (1, 100000000, 1, 1536, 0, True, 78125, 1280),
    (3, 100000000, 1, 1536, 0, True, 78125, 1280),
    (3, 100000000, 1, 1536, 0, False, 87337, 1145),
    (2, 20000000, 1, 6144, 0, True, 19532, 1024),
    (64, 312500, 1, 2048, 0, True, 39063, 8),
    (1, 30000000, 2, 512, 3, True, 131005, 229),
]


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_key_plan_table(tmp_path):
    exe = str(tmp_path / "key_plan_print")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(REPO, "tools", "key_plan_print.cpp"),
                    "-o", exe], check=True)
    rows = "".join(f"{nqg} {nslots} {rb} {rowb} {spans} {int(whole)}\n" for nqg, nslots, rb, rowb, spans, whole, _, _ in TABLE)
    out = subprocess.run([exe], input=rows, capture_output=True, text=True, check=True).stdout.split("\n")
    got = [tuple(int(x) for x in line.split()) for line in out if line]
    assert len(got) == len(TABLE)
    for row, plan in zip(TABLE, got):
        print(row[:6], "->", plan)
        assert plan == row[6:], f"key_plan{row[:6]} = {plan}, expected {row[6:]}"
