"""The entry points outside svo_process -- svo_lk_track, svo_gftt_detect, the resident KLT front end with its top-up, RANSAC gate,
prediction and stereo re-association -- held to a table recorded with the parent of the commit that moved them out of svo_api.hip
(tests/golden/frontend_census.json, written by tests/golden/make_frontend_census.py): every call sequence lists the kernel-time names it
listed, launches what it launched, returns the statuses it returned and leaves the bytes it left, and every refused call is refused
with the status and text it was refused with, before anything is enqueued."""
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_frontend_census as F                                # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def table():
    with open(F.TABLE) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def census():
    """every row and refusal, run once"""
    return F.census()


def test_the_table_holds_every_row(table):
    assert sorted(table["rows"]) == sorted(F.ROWS) and len(F.ROWS) >= 30
    assert sorted(table["refusals"]) == sorted(F.REFUSALS) and len(F.REFUSALS) >= 11
    assert table["recorded_with"]


def test_the_parent_agreed_with_itself_on_most_hashes(table):
    """a part the two recording runs differed on is null in the table and is not compared: at most one part in four"""
    assert F.null_share(table["rows"]) <= F.MAX_NULL_SHARE == 0.25


@pytest.mark.parametrize("name", list(F.ROWS))
def test_listing_launches_facts_and_bytes(table, census, name):
    want, got = table["rows"][name], census["rows"][name]
    print(name, got)
    assert "error" not in got, got
    assert got["listing"] == want["listing"]
    assert got["calls"] == want["calls"]
    assert got["facts"] == want["facts"]
    assert sorted(got["sha"]) == sorted(want["sha"])
    for part, h in want["sha"].items():
        assert h is None or got["sha"][part] == h, part


@pytest.mark.parametrize("name", list(F.REFUSALS))
def test_refusals_keep_their_status_and_text(table, census, name):
    want, got = table["refusals"][name], census["refusals"][name]
    print(name, got)
    assert "error" not in got, got
    assert (got["rc"], got["text"]) == (want["rc"], want["text"])
    assert got["rc"] < 0 and got["enqueued"] == 0
