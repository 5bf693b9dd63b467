"""Image content and frame layouts the synthetic world, the golden sequence and white noise never produce (TEST INFRASTRUCTURE).

Content: structured images whose detector output is full of TIED Harris responses, repeated descriptors, saturated pixels and
FAST scores exactly on the threshold, so that the tie rules of the parallel kernels (score bins, (response desc, position asc),
NMS orders, first minimum of the matchers) are decided on whole frames.  tests/test_image_content_cpu.py pins, from the oracle
alone, that the generators keep these properties.

Layout: `place` writes images into ONE device buffer of random poison bytes at any stride and byte offset, the way a caller's
memory looks to SVO_FLAG_DEVICE_IMAGES (crops, side-by-side stereo frames, odd widths held contiguously), always with poison
around them: an out-of-contract read shows up as a wrong result, never as a fault.

Plain functions, numpy only (`place` imports torch when called)."""
import numpy as np

GUARD = 4096                  # poison bytes kept before the first row and after data + h * stride of every placed image


def _blocks(rng, w, h, block, values):
    """random choice of `values` per block x block cell"""
    nby, nbx = (h + block - 1) // block, (w + block - 1) // block
    cells = np.asarray(values, np.uint8)[rng.randint(0, len(values), (nby, nbx))]
    return np.ascontiguousarray(np.kron(cells, np.ones((block, block), np.uint8))[:h, :w])


def periodic(w, h, seed=0, tile=64):
    """a smoothed random tile x tile texture (wrap-around box blur: the tile is seamless), contrast stretched to 0..255, repeated"""
    rng = np.random.RandomState(seed)
    t = rng.randint(0, 256, (tile, tile)).astype(np.float64)
    for axis in (0, 1):
        t = (np.roll(t, -1, axis) + t + np.roll(t, 1, axis)) / 3.0
    t = np.clip((t - t.mean()) * (3.0 * 255.0 / (t.max() - t.min())) + 128.0, 0, 255)
    t = np.floor(t + 0.5).astype(np.uint8)
    return np.ascontiguousarray(np.tile(t, ((h + tile - 1) // tile, (w + tile - 1) // tile))[:h, :w])


def mirror(w, h, seed=0, block=16):
    """a random grey block image | its left-right flip (w even): every corner has a mirror twin with the same response"""
    assert w % 2 == 0
    rng = np.random.RandomState(seed)
    half = _blocks(rng, w // 2, h, block, list(range(16, 256, 16)))
    return np.ascontiguousarray(np.hstack([half, half[:, ::-1]]))


def binary_blocks(w, h, seed=0, block=16):
    """random 0 / 255 blocks: saturated pixels, FAST scores of 254, a few distinct corner shapes"""
    return _blocks(np.random.RandomState(seed), w, h, block, [0, 255])


def checker(w, h, seed=0, block=8):
    """0 / 255 checkerboard (the seed moves its phase)"""
    oy, ox = np.random.RandomState(seed).randint(0, block, 2)
    yy, xx = np.mgrid[0:h, 0:w]
    return ((((yy + oy) // block + (xx + ox) // block) & 1) * 255).astype(np.uint8)


def threshold_edge(w, h, seed=0, th=20, block=10):
    """blocks whose grey values differ by exactly th, th + 1 and 2 th + 1: level-0 FAST scores sit on the threshold itself.  Upper
    half around base 100, lower half around bases 0 and 255 - (2 th + 1), saturated ends included.  The corners of perfect blocks
    form plateaus of equal scores, which the strict 3x3 NMS removes at level 0 altogether; so half of the blocks also carry a
    single-pixel dot in their centre, th or th + 1 away from the block's grey value: a dot at th + 1 is an isolated level-0 corner
    of score exactly th (the lowest a corner can have, hundreds of them with the same Harris response), a dot at th is none"""
    rng = np.random.RandomState(seed)
    top = _blocks(rng, w, h // 2, block, [100, 100 + th, 100 + 2 * th + 1])
    lo = 255 - (2 * th + 1)
    bottom = _blocks(rng, w, h - h // 2, block, [0, th, 2 * th + 1, lo, lo + th, 255])
    for half in (top, bottom):
        for by in range(0, half.shape[0] - block + 1, block):
            for bx in range(0, w - block + 1, block):
                if rng.rand() < 0.5:
                    y, x = by + block // 2, bx + block // 2
                    v = int(half[y, x])
                    deltas = [d for d in (th, th + 1, -th, -(th + 1)) if 0 <= v + d <= 255]
                    half[y, x] = v + deltas[rng.randint(len(deltas))]
    return np.ascontiguousarray(np.vstack([top, bottom]))


CONTENTS = {"periodic": periodic, "mirror": mirror, "binary_blocks": binary_blocks, "checker": checker, "threshold_edge": threshold_edge}
TIE_CONTENTS = ("periodic", "mirror", "binary_blocks", "checker")       # the tie floor of the CPU guard applies to these
TIE_FLOOR = 100                                                          # tied responses among the raw keypoints of a 640x480 frame, 750 requested


def right_of(img, d):
    """the right image of a fronto-parallel scene: the left one rolled by -d px"""
    return np.ascontiguousarray(np.roll(img, -int(d), axis=1))


def moved(img, dx, dy):
    """a following frame: integer roll"""
    return np.ascontiguousarray(np.roll(np.roll(img, int(dy), axis=0), int(dx), axis=1))


def tied_responses(kps):
    """keypoints that share their Harris response with another keypoint of the same pyramid level"""
    key = np.stack([kps["octave"].astype(np.int64), kps["response"].view(np.uint32).astype(np.int64)], 1)
    _, inv, cnt = np.unique(key, axis=0, return_inverse=True, return_counts=True)
    return int((cnt[inv.reshape(-1)] > 1).sum())


def duplicate_descriptors(desc):
    """descriptors that repeat an earlier one"""
    return int(len(desc) - len(np.unique(desc, axis=0))) if len(desc) else 0


def place(images, stride, base_offsets, seed=0):
    """One CUDA uint8 buffer of random poison bytes; images[i] ([h, w] or [h, w, 3] uint8) written as h rows `stride` bytes apart,
    its first byte base_offsets[i] bytes after a 256-aligned slot.  Every image has at least GUARD poison bytes before its first row
    and after data + h * stride, the last one too: no image ends where the allocation ends.
    Returns (device addresses, the torch buffer -- keep it alive --, host copy of the buffer as written)."""
    import torch
    assert len(images) == len(base_offsets)
    starts, off = [], 0
    for img, bo in zip(images, base_offsets):
        rowbytes = img.shape[1] * (img.shape[2] if img.ndim == 3 else 1)
        assert img.dtype == np.uint8 and stride >= rowbytes and 0 <= bo < 256
        start = (off + GUARD + 255) // 256 * 256 + bo
        starts.append(start)
        off = start + img.shape[0] * stride
    total = (off + GUARD + 255) // 256 * 256 + 256
    host = np.random.RandomState(seed).randint(0, 256, total).astype(np.uint8)
    for img, start in zip(images, starts):
        h = img.shape[0]
        rows = np.ascontiguousarray(img).reshape(h, -1)
        np.lib.stride_tricks.as_strided(host[start:], (h, rows.shape[1]), (stride, 1))[:] = rows
        assert start >= GUARD and start + h * stride + GUARD <= total
    buf = torch.from_numpy(host).cuda()
    torch.cuda.synchronize()
    base = buf.data_ptr()
    assert base % 256 == 0, "the allocator no longer returns 256-aligned blocks: the alignment cases would not be what they say"
    return [base + s for s in starts], buf, host.copy()


def assert_untouched(buf, host):
    """nothing wrote the caller's memory: image rows, padding and poison all still hold what was placed"""
    import torch
    torch.cuda.synchronize()
    now = buf.cpu().numpy()
    bad = np.flatnonzero(now != host)
    assert bad.size == 0, "caller memory was written: %d bytes, first at offset %d" % (bad.size, bad[0])
