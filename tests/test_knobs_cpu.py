"""The run-time knobs have one home: stereo_vo_amd/csrc/svo_knobs.cpp parses every SVO_* environment variable, once per context, and
svo_knobs.hpp names the SVO_DEBUG_MODE values.  Three checks on the sources that keep it that way (the parsing rules themselves are held
by tools/knobs_check.cpp, `make hostcheck`).  No GPU, nothing is built."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "stereo_vo_amd", "csrc")


def _read(path):
    with open(path, encoding="utf-8") as f:
        return f.read()


def _sources():
    for d in (CSRC, os.path.join(ROOT, "include")):
        for name in sorted(os.listdir(d)):
            if name.endswith((".hip", ".h", ".hpp", ".cpp")):
                yield os.path.join(d, name)


def test_only_the_knobs_unit_and_roctx_read_the_environment():
    """`getenv` occurs in svo_knobs.cpp and inside the RoctxApi block of svo_api.hip (whether a profiler library is loaded into the
    process), nowhere else under stereo_vo_amd/csrc and include"""
    seen = {}
    for path in _sources():
        text, name = _read(path), os.path.basename(path)
        if name == "svo_api.hip":                           # cut the RoctxApi struct out: from its head to the accessor that follows it
            a, b = text.index("struct RoctxApi {"), text.index("RoctxApi& roctx_api()")
            assert a < b and text[a:b].count("getenv") == 2, "the RoctxApi block is not where this test expects it"
            text = text[:a] + text[b:]
        if "getenv" in text:
            seen[name] = text.count("getenv")
    assert list(seen) == ["svo_knobs.cpp"], seen


def test_the_knob_table_of_integration_md_lists_what_is_read():
    """every SVO_* name svo_knobs.cpp asks for is in the first column of INTEGRATION.md's knob table, and every name there is asked for by
    svo_knobs.cpp or is SVO_ROCTX"""
    read = set(re.findall(r'"(SVO_[A-Z0-9_]+)"', _read(os.path.join(CSRC, "svo_knobs.cpp"))))
    assert len(read) == 12, sorted(read)
    doc = _read(os.path.join(ROOT, "INTEGRATION.md"))
    a = doc.index("## Environment knobs of `libsvo_hip.so`")
    assert "read once per context, at `svo_create`" in doc[a:doc.index("\n", a)]
    rows = []
    for line in doc[a:].split("\n")[1:]:
        if line.startswith("|"):
            rows.append(line)
        elif rows:
            break                                           # the table has ended
    listed = set()
    for row in rows[2:]:                                    # (header and rule lines first)
        first = row.split("|")[1]
        listed.update(re.findall(r"`(SVO_[A-Z0-9_]+)`", first))
    assert read <= listed, sorted(read - listed)
    assert listed - read == {"SVO_ROCTX"}, sorted(listed - read)


def test_no_kernel_file_compares_a_debug_mode_with_a_number():
    """debug_mode / dbg are compared with the names of svo_knobs.hpp (DebugMode), never with a literal"""
    left = re.compile(r"\b(?:debug_mode|dbg|dm)\s*(?:==|!=|<=|>=|<|>)\s*-?\d")
    right = re.compile(r"(?<![\w.])-?\d+\s*(?:==|!=|<=|>=|<|>)\s*(?:\w+(?:\.|->))*(?:debug_mode|dbg|dm)\b")
    found = []
    for path in _sources():
        if not path.endswith(".hip"):
            continue
        for i, line in enumerate(_read(path).split("\n"), 1):
            if left.search(line) or right.search(line):
                found.append("%s:%d: %s" % (os.path.basename(path), i, line.strip()[:120]))
    assert not found, found
