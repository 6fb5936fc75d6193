"""conv3x3_bwd_plan (csrc/conv3x3_plan.cc): the forward's geometry with C and N
exchanged, its eligibility range and a `native` table of its own."""

import pytest

from torch_cgx_amd import _C

# (batch, H, W, C of dX, N of dY, max_workgroups): the shapes of
# test_gpu_conv3x3_bwd.py, three near misses of kNativeBwd3x3 and the table
# itself, the bottleneck problems of ResNet-50 (all four measured faster)
RESNET = [(256, 56, 56, 64, 64, 0), (256, 28, 28, 128, 128, 0),
          (256, 14, 14, 256, 256, 0), (256, 7, 7, 512, 512, 0)]
GRID = [(2, 1, 1, 64, 64, 0), (2, 3, 5, 64, 64, 0), (3, 7, 7, 64, 128, 0),
        (2, 7, 7, 128, 64, 0), (2, 3, 56, 64, 64, 0), (2, 5, 5, 256, 256, 0),
        (2, 3, 3, 512, 512, 0), (5, 12, 12, 64, 64, 2),
        (64, 14, 14, 64, 128, 7), (128, 56, 56, 64, 64, 0),
        (256, 28, 27, 128, 128, 0), (256, 14, 14, 256, 512, 0)] + RESNET


@pytest.mark.parametrize("shape", GRID, ids=lambda s: "x".join(map(str, s)))
def test_geometry_is_the_forwards_with_c_and_n_exchanged(shape):
    b, h, w, c, n, wg = shape
    p = _C.conv3x3_bwd_plan(b, h, w, c, n, wg)
    f = _C.conv3x3_fwd_plan(b, h, w, n, c, wg)
    assert p["eligible"] and p["rows"] == b * h * w
    assert p["ntiles"] * p["bn"] == c and p["nchunks"] * p["kc"] == n
    assert p["resident"] == (n == 64)  # both instantiations are in GRID
    assert p["pstride"] == 0 and p["partial_floats"] == 0  # no partials
    for key in ("ntiles", "nchunks", "resident", "row_tiles", "strip_rows",
                "xvecs", "splits", "grid", "tiles_per_split", "lds_bytes"):
        assert p[key] == f[key], key
    assert p["lds_bytes"] <= p["lds_budget"] == 160 * 1024
    assert p["native"] == (shape in RESNET)


def test_what_is_not_eligible():
    for bad in ((2, 4, 4, 32, 64), (2, 4, 4, 64, 96), (2, 4, 4, 1024, 64),
                (2, 4, 4, 64, 1024), (0, 4, 4, 64, 64), (2, 0, 4, 64, 64),
                (2, 4, 0, 64, 64), (1, 1, 1, 64, 64), (2, 4, 160, 64, 64),
                (1 << 12, 1 << 7, 1 << 6, 64, 64)):
        p = _C.conv3x3_bwd_plan(*bad)
        assert not p["eligible"] and not p["native"], bad
    assert _C.conv3x3_bwd_plan(1, 2, 159, 512, 512)["eligible"]
