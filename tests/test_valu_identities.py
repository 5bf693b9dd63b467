"""The integer identities behind the instruction cuts in k_resize and k_fast (stereo_vo_amd/csrc/k_detect.hip), CPU, numpy only.

Each test evaluates the formula as the kernel wrote it BEFORE the cut and as it writes it now, in the kernel's own number
formats (packed 16-bit halves, 32-bit wrap-around, unsigned saturation), over every input or a dense set of them.  They guard
the reasoning; that the compiled kernels compute the same pyramid and the same candidates is what the GPU parity tests check.
"""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

U16 = np.uint16
M32 = np.uint64(0xFFFFFFFF)


# ---------------------------------------------------------------------------------------------------------------------------
# A. k_resize: dot2 of (pixel << 8) with (weight << 4), high word  ==  (dot2 of pixel with weight) >> 4
# ---------------------------------------------------------------------------------------------------------------------------
def _perm(s0, s1, sel):
    """v_perm_b32 D = perm(S0, S1, sel): result byte i = byte sel[i] of {S0 : S1} (S1 = bytes 0-3), a selector byte of 0x0c gives 0x00"""
    window = [(s1 >> (8 * i)) & 0xFF for i in range(4)] + [(s0 >> (8 * i)) & 0xFF for i in range(4)]
    out = 0
    for i in range(4):
        b = (sel >> (8 * i)) & 0xFF
        assert b < 8 or b == 0x0c
        out |= (0 if b == 0x0c else window[b]) << (8 * i)
    return out


def _udot2(a, b):
    """v_dot2_u32_u16 without clamp: lo(a) * lo(b) + hi(a) * hi(b) modulo 2^32 (arrays of uint64 holding 32-bit words)"""
    return ((a & np.uint64(0xFFFF)) * (b & np.uint64(0xFFFF)) + (a >> np.uint64(16)) * (b >> np.uint64(16))) & M32


def test_resize_tap_selectors_put_the_pixels_into_the_high_bytes():
    rng = np.random.default_rng(5)
    for _ in range(200):
        lo, hi = int(rng.integers(0, 1 << 32)), int(rng.integers(0, 1 << 32))
        for o in range(6):                                       # tap offsets inside the thread's 8-byte window: 0 .. 5
            old = _perm(hi, lo, 0x0c010c00 + o * 0x00010001)
            new = _perm(hi, lo, 0x010c000c + o * 0x01000100)
            window = lo | (hi << 32)
            p0, p1 = (window >> (8 * o)) & 0xFF, (window >> (8 * o + 8)) & 0xFF
            assert old == p0 | (p1 << 16)
            assert new == (p0 << 8) | (p1 << 24) == old << 8


def test_resize_scaled_dot_product_high_word_is_the_row_sum_cut_by_four_bits():
    p0 = np.repeat(np.arange(256, dtype=np.uint64), 256)
    p1 = np.tile(np.arange(256, dtype=np.uint64), 256)
    t_old = p0 | (p1 << np.uint64(16))                           # u16 pair (p0, p1)
    t_new = (p0 << np.uint64(8)) | (p1 << np.uint64(24))         # the pixels in the high bytes
    worst = 0
    for a1 in range(2049):
        a0 = 2048 - a1
        w_old = np.uint64(a0 | (a1 << 16))                       # the table word: a0 | a1 << 16
        w_new = np.uint64(((a0 | (a1 << 16)) << 4) & 0xFFFFFFFF) # xw[] = word << 4 in 32 bits
        assert int(w_new) & 0xFFFF == a0 << 4 and int(w_new) >> 16 == a1 << 4        # no bit crosses the halves or leaves the word
        top = _udot2(t_old, w_old)
        scaled = _udot2(t_new, w_new)
        assert np.array_equal(scaled, top * np.uint64(4096))     # exactly 4096 x the row sum: nothing wrapped
        assert np.array_equal(scaled >> np.uint64(16), top >> np.uint64(4))
        worst = max(worst, int(scaled.max()))
    assert worst == 4096 * 255 * 2048 < 1 << 31                  # the 32-bit bound, with a bit to spare


def test_resize_scaled_dot_product_with_independently_rounded_weights():
    # the table rounds a0 and a1 separately: a0 + a1 may be 2047 or 2049.  Still below 2^32, still exact.
    p = np.arange(256, dtype=np.uint64)
    p0, p1 = np.repeat(p, 256), np.tile(p, 256)
    for a1 in (0, 1, 1023, 1024, 1025, 2047, 2048):
        for a0 in {max(0, 2047 - a1), 2048 - a1, min(2048, 2049 - a1)}:
            w = (a0 | (a1 << 16))
            top = _udot2(p0 | (p1 << np.uint64(16)), np.uint64(w))
            scaled = _udot2((p0 << np.uint64(8)) | (p1 << np.uint64(24)), np.uint64((w << 4) & 0xFFFFFFFF))
            assert np.array_equal(scaled, top * np.uint64(4096)) and np.array_equal(scaled >> np.uint64(16), top >> np.uint64(4))


# ---------------------------------------------------------------------------------------------------------------------------
# B1. fast_score_lds: the centre added once to the network's result instead of to each of the sixteen inputs
# ---------------------------------------------------------------------------------------------------------------------------
def _fast_score(p, c, th, add_first):
    """p: (n, 16) circle pixels, c: (n,) centres -> the kernel's score, in wrapping int16 halves (x = bright side, y = dark side)"""
    prod = (p.astype(np.int32) * np.int32(-65535))               # __mul24(p, -65535): halves (p, -p)
    halves = prod.view(np.int16).reshape(p.shape[0], 16, 2).copy()
    assert np.array_equal(halves[:, :, 0], p.astype(np.int16)) and np.array_equal(halves[:, :, 1], -p.astype(np.int16))
    K = np.stack([(-c).astype(np.int16), c.astype(np.int16)], axis=1)                # (-c, c)
    v = halves + K[:, None, :] if add_first else halves
    s0, s1, p0, p1 = [None] * 8, [None] * 8, [None] * 8, [None] * 8
    s0[7], s1[7], p0[0], p1[0] = v[:, 7], v[:, 15], v[:, 0], v[:, 8]
    for j in range(6, -1, -1):
        s0[j], s1[j] = np.minimum(s0[j + 1], v[:, j]), np.minimum(s1[j + 1], v[:, 8 + j])
    for j in range(1, 8):
        p0[j], p1[j] = np.minimum(p0[j - 1], v[:, j]), np.minimum(p1[j - 1], v[:, 8 + j])
    m = np.minimum(s0[0], p1[0])
    for i in range(1, 8):
        m = np.maximum(m, np.minimum(s0[i], p1[i]))
    for i in range(8):
        m = np.maximum(m, np.minimum(s1[i], p0[i]))
    if not add_first:
        assert np.abs(m.astype(np.int32)).max() <= 255
        m = m + K                                                # int16, wraps like v_pk_add_i16 (it cannot: |m| <= 255, |K| <= 255)
    best = np.maximum(m[:, 0], m[:, 1]).astype(np.int32)
    return np.where(best > th, best - 1, 0)


def test_fast_score_centre_added_once():
    rng = np.random.default_rng(11)
    n = 60000
    p = rng.integers(0, 256, size=(n, 16))
    c = rng.integers(0, 256, size=n)
    # real corners as well as noise: arcs of bright / dark pixels of random length and start around a random centre
    arc = rng.integers(0, 256, size=(n, 16))
    start, length = rng.integers(0, 16, size=n), rng.integers(7, 13, size=n)
    idx = (np.arange(16)[None, :] - start[:, None]) % 16
    sign = np.where(rng.integers(0, 2, size=n) == 1, 1, -1)
    lift = rng.integers(1, 120, size=n)
    arc = np.where(idx < length[:, None], np.clip(c[:, None] + sign[:, None] * (lift[:, None] + arc % 30), 0, 255), np.clip(c[:, None] + (arc % 9) - 4, 0, 255))
    extremes = np.array([[0] * 16, [255] * 16, [0] * 16, [255] * 16, [0, 255] * 8, [255] * 9 + [0] * 7, [0] * 9 + [255] * 7])
    ec = np.array([0, 255, 255, 0, 128, 0, 255])
    P = np.concatenate([p, arc, extremes]); C = np.concatenate([c, c, ec])
    seen_corner = 0
    for th in (0, 1, 7, 20, 60, 254):
        old = _fast_score(P, C, th, add_first=True)
        new = _fast_score(P, C, th, add_first=False)
        assert np.array_equal(old, new)
        seen_corner += int((old > 0).sum())
    assert seen_corner > 10000                                   # the set does exercise the scoring branch


# ---------------------------------------------------------------------------------------------------------------------------
# B2. quick_half: sub_sat(b, add_sat(cc, t2)) | sub_sat(sub_sat(cc, t2), d)  against  sub_sat(max(sub_sat(b, cc), sub_sat(cc, d)), t2)
# ---------------------------------------------------------------------------------------------------------------------------
def _sub_sat(a, b):
    """unsigned 16-bit saturating a - b (v_pk_sub_u16 clamp), elementwise with broadcasting"""
    return np.maximum(a, b) - b


def _add_sat(a, b):
    s = a.astype(np.uint32) + np.uint32(b)
    return np.minimum(s, 65535).astype(U16)


def _quick_half_case(low_b, low_c, low_d):
    hi = (np.arange(256, dtype=np.uint32) << 8)
    b = (hi | low_b).astype(U16)[:, None, None]
    cc = (hi | low_c).astype(U16)[None, :, None]
    d = (hi | low_d).astype(U16)[None, None, :]
    # the new form's inner part does not depend on the threshold
    inner = np.maximum(_sub_sat(b, cc), _sub_sat(cc, d))         # (256, 256, 256)
    mism = 0
    for th in range(256):
        t2 = U16(th << 8)
        old = _sub_sat(b, _add_sat(cc, t2)) | _sub_sat(_sub_sat(cc, t2), d)
        new = _sub_sat(inner, t2)
        mism += int(np.count_nonzero((old != 0) != (new != 0)))
    return mism


def test_quick_half_four_operation_form_flags_the_same_positions():
    # every (b, cc, d) high byte x every threshold 0..255 (packed domain: t2 = th << 8) x low bytes that order the ties every way
    lows = [(0, 0, 0), (0xFF, 0xFF, 0xFF), (0xFF, 0, 0xFF), (0, 0xFF, 0), (0xFF, 0, 0), (0, 0, 0xFF), (0x80, 0x7F, 0x81), (0x01, 0xFE, 0x37)]
    with ThreadPoolExecutor(max_workers=max(1, min(4, os.cpu_count() or 1))) as ex:
        res = list(ex.map(lambda l: _quick_half_case(*l), lows))
    assert res == [0] * len(lows)


def test_quick_half_saturation_corners():
    # cc + t2 beyond 65535 and cc < t2, full 16-bit values, all three operands random
    rng = np.random.default_rng(3)
    n = 400000
    b, cc, d = (rng.integers(0, 65536, size=n).astype(U16) for _ in range(3))
    edge = np.array([0, 1, 0xFF, 0x100, 0x7FFF, 0x8000, 0xFEFF, 0xFF00, 0xFFFE, 0xFFFF], dtype=U16)
    g = np.array(np.meshgrid(edge, edge, edge, indexing="ij")).reshape(3, -1)
    b, cc, d = np.concatenate([b, g[0]]), np.concatenate([cc, g[1]]), np.concatenate([d, g[2]])
    for th in range(256):
        t2 = U16(th << 8)
        old = _sub_sat(b, _add_sat(cc, t2)) | _sub_sat(_sub_sat(cc, t2), d)
        new = _sub_sat(np.maximum(_sub_sat(b, cc), _sub_sat(cc, d)), t2)
        assert np.array_equal(old != 0, new != 0), th


# ---------------------------------------------------------------------------------------------------------------------------
# B3. the verdict masks: me |= fe << g for g = 0 .. 7  against  me = (me << 1) | fe for g = 7 .. 0
# ---------------------------------------------------------------------------------------------------------------------------
def test_verdict_masks_built_by_shift_and_or_have_the_same_bits():
    ROWS = 8
    pat = np.arange(1 << 16, dtype=np.uint32)                    # bit g: low-half verdict of row g, bit 8 + g: high-half verdict
    f = [((pat >> g) & 1) | (((pat >> (8 + g)) & 1) << 16) for g in range(ROWS)]     # v_pk_min_u16(x, 1): 0 / 1 per half
    old = np.zeros_like(pat)
    for g in range(ROWS):
        old |= f[g] << g
    new = f[ROWS - 1].copy()
    for g in range(ROWS - 2, -1, -1):
        new = ((new << 1) | f[g]).astype(np.uint32)              # v_lshl_or_b32 new, new, 1, f
    assert np.array_equal(old, new)
    # the layout entry_of() decodes: bit g = position 0 (or 1) of row g, bit 16 + g = position 2 (or 3)
    assert np.array_equal(new & 0xFF, pat & 0xFF) and np.array_equal((new >> 16) & 0xFF, pat >> 8) and not (new & 0xFF00FF00).any()
    # both masks together: m = me | mo << 8 never collides
    rng = np.random.default_rng(9)
    i, j = rng.integers(0, 1 << 16, size=100000), rng.integers(0, 1 << 16, size=100000)
    m = new[i] | (new[j] << 8)
    assert np.array_equal(m, old[i] | (old[j] << 8))
    pop = np.array([bin(x).count("1") for x in range(1 << 16)])
    assert np.array_equal(np.array([bin(int(x)).count("1") for x in m[:2000]]), pop[i[:2000]] + pop[j[:2000]])
