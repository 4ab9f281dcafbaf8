"""The argument checks of the mdpt_post_* entry points refuse what they refused, word for word: every case of tests/post_refusal_cases.py against
tests/golden/post_refusals.json, which tests/golden/gen_post_refusals.py recorded at the commit its header names. The checks return before any launch,
so nothing here needs a GPU; the accepted *_scratch_bytes queries pin the size arithmetic."""
import json
import os

import pytest

from muggled_dpt_amd import native
from tests import post_refusal_cases as table

with open(os.path.join(os.path.dirname(__file__), "golden", "post_refusals.json")) as _fh:
    GOLDEN = json.load(_fh)


def test_the_table_and_the_golden_file_hold_the_same_cases():
    names = [name for name, _, _ in table.CASES]
    assert len(set(names)) == len(names) == GOLDEN["header"]["refusals"] and set(names) == set(GOLDEN["refusals"])
    queries = [name for name, _, _ in table.ACCEPTED]
    assert len(set(queries)) == len(queries) == GOLDEN["header"]["accepted"] and set(queries) == set(GOLDEN["accepted"])
    assert len(GOLDEN["header"]["commit"]) == 40
    assert all(code == -1 for code, _ in GOLDEN["refusals"].values()) and all(code == 0 and size > 0 for code, size in GOLDEN["accepted"].values())
    entries = {entry for _, entry, _ in table.CASES}
    assert entries == set(table.GOOD) == {s for s in native.SYMBOLS if s.startswith("mdpt_post_")} and len(entries) == GOLDEN["header"]["entry_points"]


@pytest.mark.parametrize("entry", sorted(table.GOOD))
def test_every_refusal_of_an_entry_point_is_the_recorded_one(entry):
    lib = native.load()
    cases = [(name, changed) for name, e, changed in table.CASES if e == entry]
    assert cases
    for name, changed in cases:
        code, message, _ = table.run(lib, entry, changed)
        assert [code, message] == GOLDEN["refusals"][name], name


def test_accepted_scratch_queries_return_the_recorded_sizes():
    lib = native.load()
    for name, entry, changed in table.ACCEPTED:
        code, _, size = table.run(lib, entry, changed)
        assert [code, size] == GOLDEN["accepted"][name], name
