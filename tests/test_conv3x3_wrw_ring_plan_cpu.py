"""The geometry of conv3x3_wrw_ring (csrc/conv3x3_plan.h) on the host: the
fill of a stage by loads direct to LDS replayed against the image layout
(wrw_cell in csrc/wrw_image.h) and against the `live` predicate of
conv3x3_wrw's register staging (conv3x3_load in csrc/conv3x3_kernels.hip),
both written out again here."""

import functools

import pytest

from torch_cgx_amd import _C

STAGES = (2, 3)
# (batch, H, W, C, N)
BENCH = [(256, 56, 56, 64, 64), (256, 28, 28, 128, 128),
         (256, 14, 14, 256, 256), (256, 7, 7, 512, 512)]
# the four widths at a small batch, one with a batch that does not fill the
# last group of images, one whose H is no multiple of hr
SMALL = [(3, 56, 56, 64, 64), (3, 28, 28, 64, 128), (3, 14, 14, 128, 64),
         (11, 7, 7, 64, 64), (2, 30, 28, 64, 64), (5, 3, 5, 64, 64)]


def _plan(shape, stages):
    return _C.conv3x3_wrw_ring_plan(*shape, 0, stages)


def wrw_cell64(r, u):
    lin = r * 2 + u
    return 256 * (lin >> 2) + 64 * ((lin & 3) ^ ((r >> 1) & 1))


def wrw_row(p, shape, group, t):
    """conv3x3_wrw_row."""
    batch, h = shape[0], shape[1]
    if t < 0 or t >= p["group_rows"]:
        return -1
    image, hh = (divmod(t, h + 1) if p["images"] > 1 else (0, t))
    b = group * p["images"] + image
    return b * h + hh if hh < h and b < batch else -1


def live_pixel(p, shape, chunk, is_x, pos):
    """What conv3x3_load puts at position `pos`: the pixel, or -1 for zeros."""
    w = shape[2]
    group, ci = divmod(chunk, p["chunks_per_image"])
    t0 = ci * p["hr"] - is_x
    strip = p["strip_x"] if is_x else p["strip_dy"]
    rr, col = divmod(pos, p["pitch"])
    col -= is_x
    row = wrw_row(p, shape, group, t0 + rr)
    live = (pos < strip and row >= 0 and rr < p["hr"] + 2 * is_x
            and 0 <= col < w)
    return row * w + col if live else -1


@functools.lru_cache(maxsize=None)
def _fill(shape, stages, chunk):
    return _C.conv3x3_wrw_ring_fill(*shape, 0, stages, chunk).reshape(-1, 5) \
        .tolist()


def _chunks(p):
    """First, middle and last chunk of an image (or group) and the last of
    all, where the batch ends."""
    cpi = p["chunks_per_image"]
    return sorted({0, cpi // 2, cpi - 1, p["chunks"] - 1,
                   max(0, p["chunks"] - cpi)})


@pytest.mark.parametrize("stages", STAGES)
@pytest.mark.parametrize("shape", SMALL + BENCH[:1] + BENCH[3:], ids=str)
def test_fill_is_the_image_of_the_strips(shape, stages):
    p = _plan(shape, stages)
    assert p["eligible"] and p["bn"] == p["bk"] == 64
    pixels = shape[0] * shape[1] * shape[2]
    for chunk in _chunks(p):
        entries = _fill(shape, stages, chunk)
        assert len(entries) == p["stage_bytes"] // 16
        seen = set()
        for byte, is_x, pos, vec, pixel in entries:
            image = p["dy_glds"] * 4096 if is_x else 0
            assert byte == image + wrw_cell64(pos, vec >> 2) + 16 * (vec & 3)
            assert (is_x, pos, vec) not in seen
            seen.add((is_x, pos, vec))
            assert pixel == live_pixel(p, shape, chunk, is_x, pos)
            assert -1 <= pixel < pixels
        # every byte of the stage exactly once, so every position below the
        # reach strip_dy + 2P + 1 <= strip_x of the last tap as well
        assert sorted(e[0] for e in entries) == list(
            range(0, p["stage_bytes"], 16))
        assert p["strip_dy"] + 2 * p["pitch"] + 2 <= p["strip_x"]
        for is_x, strip in ((0, p["strip_dy"]), (1, p["strip_x"])):
            assert all((is_x, pos, v) in seen
                       for pos in range(strip) for v in range(8))


def test_the_cases_have_the_zeros_they_are_for():
    shape = SMALL[4]                      # H = 30 in chunks of hr rows
    p = _plan(shape, 2)
    assert p["images"] == 1 and p["chunks_per_image"] >= 3
    assert shape[1] % p["hr"]             # rows past the image
    last = [e for e in _fill(shape, 2, p["chunks_per_image"] - 1) if not e[1]]
    short = shape[1] - (p["chunks_per_image"] - 1) * p["hr"]
    assert sum(e[4] >= 0 for e in last) == short * shape[2] * 8
    p7 = _plan(SMALL[3], 2)               # groups of images, batch 11
    assert p7["images"] > 1 and SMALL[3][0] % p7["images"]
    tail = [e for e in _fill(SMALL[3], 2, p7["chunks"] - 1) if not e[1]]
    assert sum(e[4] >= 0 for e in tail) == \
        (SMALL[3][0] % p7["images"]) * 49 * 8


@pytest.mark.parametrize("stages", STAGES)
@pytest.mark.parametrize("shape", SMALL + BENCH, ids=str)
def test_limits(shape, stages):
    p = _plan(shape, stages)
    assert p["lds_bytes"] == stages * p["stage_bytes"] <= p["lds_budget"]
    assert p["stage_bytes"] == 4096 * (p["dy_glds"] + p["x_glds"])
    assert p["dy_glds"] + p["x_glds"] <= 20
    assert p["strip_dy"] % 32 == 0 and p["strip_dy"] <= 32 * p["dy_glds"]
    assert p["strip_x"] <= 32 * p["x_glds"]
    assert 1 <= p["splits"] <= p["chunks"]
    assert p["grid"] == p["splits"] * p["ntiles_n"] * p["ntiles_k"]
    assert p["chunks_per_split"] == -(-p["chunks"] // p["splits"])


def test_benchmark_problems_get_the_recorded_plans():
    """benchmarks/RESULTS.md, "Ring-staged 3x3 weight gradient"."""
    want = {2: [(4, 1, 256, 14), (7, 1, 64, 16), (14, 1, 16, 16),
                (31, 4, 4, 16)],
            3: [(2, 1, 256, 28), (5, 1, 64, 24), (7, 1, 16, 32),
                (23, 3, 4, 22)]}
    for stages, rows in want.items():
        for shape, row in zip(BENCH, rows):
            p = _plan(shape, stages)
            assert (p["hr"], p["images"], p["splits"],
                    p["chunks_per_split"]) == row
            assert p["grid"] == 256
    assert _plan(BENCH[0], 0)["stages"] == 2


def test_rejects():
    assert not _plan((2, 7, 7, 32, 64), 2)["eligible"]
    assert not _plan((2, 7, 7, 64, 1024), 2)["eligible"]
    assert not _plan((2, 7, 7, 64, 64), 4)["eligible"]
    assert not _plan((2, 7, 400, 64, 64), 2)["eligible"]
