"""The one table of kernel-time names (stereo_vo_amd/csrc/kernel_names.cpp): what svo_kernel_times can list, in its order."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ALWAYS = ["begin_frame", "resize", "fast", "select", "describe", "nms_rowsort", "hamming_lr", "match_lr_filter", "hamming_track", "track_filter",
          "ransac_hyp", "ransac_count", "track_finalize", "gauss_newton", "ransac_hyp_1", "ransac_count_1", "ransac_hyp_2", "ransac_count_2",
          "sad_patch", "match_lr_sad", "track_sad", "select_8192", "nms_rowsort_16", "hamming_lr_wide", "hamming_track_wide", "track_filter_64",
          "export_frame", "import_frame", "export_frame_win", "import_frame_win", "faster", "faster_nms", "gather_windows"]
ON_DEMAND = ["pose_covariance", "landmarks", "gftt_response", "gftt_candidates", "gftt_select", "lk_pyrdown", "lk_track", "klt_select", "klt_topup",
             "ransac_feed", "klt_prune", "klt_predict", "lk_track_row"]


def read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_one_table_lists_every_name_in_order_and_is_checked_on_the_host():
    src = read("stereo_vo_amd", "csrc", "kernel_names.cpp")
    table = re.search(r"kernel_names\[KT_COUNT\] = \{\n(.*?)\n\};", src, re.S).group(1)
    row = r'\{ (KT_[A-Z0-9_]+), "([a-z0-9_]+)", (KG_[A-Z_]+) \},'
    rows = re.findall(row, table)
    assert not re.sub(row, "", table).strip()                             # the table holds rows and nothing else
    names = [name for _, name, _ in rows]
    assert len(ALWAYS) == 33 and names == ALWAYS + ON_DEMAND
    assert len(set(names)) == len(names) and len({i for i, _, _ in rows}) == len(rows)
    assert len(names) <= 64                                               # what Context.kernel_times reads
    assert [g for _, _, g in rows[:33]] == ["KG_ALWAYS"] * 33 and "KG_ALWAYS" not in [g for _, _, g in rows[33:]]
    # the ids are declared in the order of the rows
    ids = re.search(r"enum KernelTimeId : int \{(.*?)KT_COUNT\s*\};", read("stereo_vo_amd", "csrc", "kernel_names.hpp"), re.S).group(1)
    assert re.findall(r"\bKT_[A-Z0-9_]+", re.sub(r"//[^\n]*", "", ids)) == [i for i, _, _ in rows]
    # ... and the program that holds the listing rule and the lookup to the table is part of `make hostcheck`
    mk = read("stereo_vo_amd", "csrc", "Makefile")
    assert re.search(r"^hostcheck:.*\$\(KNAMESCHECK\)", mk, re.M) and "KNAMESCHECK = ../../tools/kernel_names_check" in mk
    rule = re.search(r"^\$\(KNAMESCHECK\):.*\n\t(.*)$", mk, re.M).group(1)
    assert "-fsanitize=address,undefined" in rule and "kernel_names_check.cpp" in rule and "kernel_names.cpp" in rule
    assert "tools/kernel_names_check" in read(".gitignore").split()
    src = read("tools", "kernel_names_check.cpp")
    assert "int main()" in src and "kernel_time_listing" in src and "kernel_time_id" in src
