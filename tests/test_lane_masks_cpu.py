"""Host side of the per-lane active masks (svo_process_lanes / svo_batch_step_lanes): the binding declares and the library
exports both entry points, and the mask packing helpers of hip.py / pipeline.py turn lane lists and bool arrays into the words
the C-ABI takes -- bit l & 63 of word l >> 6 -- and back.  No GPU needed."""
import ctypes as C

import numpy as np
import pytest

from stereo_vo_amd import hip


def test_binding_declares_and_library_exports_both_entry_points():
    assert "svo_process_lanes" in hip.EXPORTS and "svo_batch_step_lanes" in hip.BATCH_EXPORTS
    L = hip.lib()
    for name in ("svo_process_lanes", "svo_batch_step_lanes"):
        f = getattr(L, name)
        assert f is not None and f.argtypes[3] == C.POINTER(C.c_uint64), name
    # no context / no batch: refused like every other entry point, before anything else is looked at
    assert L.svo_process_lanes(None, None, 15, (C.c_uint64 * 2)(1, 0)) == -2
    assert L.svo_batch_step_lanes(None, None, 0, (C.c_uint64 * 1)(1)) == -2


@pytest.mark.parametrize("n", [1, 64, 65, 128])
def test_lane_lists_to_words_and_back(n):
    nw = (n + 63) // 64
    assert hip.lane_mask_words(None, n) == [((1 << min(64, n - 64 * w)) - 1) for w in range(nw)]          # every lane
    assert hip.lane_mask_words([], n) == [0] * nw
    assert hip.lane_mask_words([n - 1], n) == [0] * (nw - 1) + [1 << ((n - 1) & 63)]
    assert hip.lane_mask_words([0, n - 1, 0], n)[0] & 1                                                     # repeats are harmless
    picks = sorted({0, n // 2, n - 1} | ({63, 64} if n > 64 else set()))
    words = hip.lane_mask_words(picks, n)
    assert len(words) == nw and hip.lane_mask_lanes(words, n) == picks
    assert sum(bin(w).count("1") for w in words) == len(picks)
    for l in picks:
        assert (words[l >> 6] >> (l & 63)) & 1
    # a bool array says the same thing; a generator and a numpy index array do too
    b = np.zeros(n, bool); b[picks] = True
    assert hip.lane_mask_words(b, n) == words and hip.lane_mask_words(list(b), n) == words
    assert hip.lane_mask_words((l for l in picks), n) == words and hip.lane_mask_words(np.array(picks, np.int64), n) == words
    assert hip.lane_mask_lanes(hip.lane_mask_words(None, n), n) == list(range(n))
    for bad in ([n], [-1], np.zeros(n + 1, bool), [0.5]):
        with pytest.raises(ValueError):
            hip.lane_mask_words(bad, n)


@pytest.mark.parametrize("lanes", [1, 64, 65, 128, 192])
def test_batch_mask_is_one_word_per_64_global_lanes(lanes):
    from stereo_vo_amd.pipeline import batch_mask, _frames
    assert batch_mask(None, lanes) is None
    picks = sorted({0, lanes - 1, lanes // 3})
    m = batch_mask(picks, lanes)
    assert len(m) == (lanes + 63) // 64 and m._type_ is C.c_uint64
    assert hip.lane_mask_lanes(list(m), lanes) == picks
    # the frame table leaves the entries of streams that sit a step out untouched (NULL pointers)
    fr = _frames([(16, 32) if g in picks else None for g in range(lanes)], 8, 4, 8)
    for g in range(lanes):
        assert (fr[g].left.data, fr[g].right.data) == ((16, 32) if g in picks else (None, None))


def test_context_reads_an_iterable_mask_once():
    """the process_* calls need the mask twice (which entries of `pairs` to skip, the words for the C call): a generator is read once"""
    c = hip.Context.__new__(hip.Context)
    c.n_lanes, c.h = 70, None
    words, idle = c._mask(l for l in (0, 64, 69))
    assert words == hip.lane_mask_words([0, 64, 69], 70) and idle == set(range(70)) - {0, 64, 69}
    assert c._mask(None) == (None, set())
