"""The launches of a frame, held to a table recorded with the parent of the commit that split svo_process into a checked call, a window
step and stage enqueues (tests/golden/launch_census.json, written by tests/golden/make_launch_census.py): every detector, NMS setting,
stage-3 / stage-4 method and call shape launches the kernels it launched before, name for name and count for count, captures and
replays the graphs it did, and is refused with the status and text it was refused with."""
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_launch_census as M                                  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def table():
    with open(M.TABLE) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def census():
    """every row and refusal, run once (the rows under SVO_DEBUG_MODE=9 in one child process that has it in its environment)"""
    return M.census_with_children()


def test_the_table_holds_every_row(table):
    assert sorted(table["rows"]) == sorted(M.row_name(r) for r in M.ROWS)
    assert sorted(table["refusals"]) == sorted(r[0] for r in M.REFUSALS)
    assert len({M.row_name(r) for r in M.ROWS}) == len(M.ROWS) >= 24


@pytest.mark.parametrize("name", [M.row_name(r) for r in M.ROWS])
def test_launches_name_for_name_and_count_for_count(table, census, name):
    want, got = table["rows"][name], census["rows"][name]
    print(name, got["calls"], got["graphs"])
    assert got["calls"] == want["calls"]
    assert got["graphs"] == want["graphs"]


def test_call_shapes_of_one_configuration_leave_equal_lanes(census):
    """one call, detect / post + rest (with and without SVO_FLAG_DETECT_SPLIT_AT_SELECT), the detect-ahead pair, debug mode 9: the same
    result records, status words and lists, byte for byte, after two frames and after four frames under graphs.  A frame run one stage
    per call leaves the same lists; its result record is the last call's own (k_begin_frame starts it anew in every call: make_launch_census.STAGED_OWN)."""
    assert M.disagreements(census["rows"]) == {}


@pytest.mark.parametrize("name", [r[0] for r in M.REFUSALS])
def test_refusals_keep_their_status_and_text(table, census, name):
    want, got = table["refusals"][name], census["refusals"][name]
    print(name, got)
    assert (got["rc"], got["text"]) == (want["rc"], want["text"])
    assert got["rc"] < 0 and got["enqueued"] == 0
