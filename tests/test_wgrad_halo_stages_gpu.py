"""Two-object LDS stages of the halo weight gradient's lean pixel loop
(csrc/kernels/wgrad_halo.hip, STG; ops.set_halo_wgrad_stages) against the
lean loop with both stages in one array, bit for bit, and against the float32
PyTorch reference with test_wgrad_halo_gpu.py's bounds.  The new loop runs two
pixel steps a turn (one per stage array) and an odd step count's last step
after it, so besides the shapes of test_wgrad_halo_lean_gpu.py (both window
forms, MT 96 and 128, the 5 x 5 layer, steps that straddle two images; the
plan's own split and seven ranges) there are splits at which a workgroup runs
exactly one, two and three steps, in the full-row and in the segment form, and
one workgroup per tile with an even count over several image wraps.  Every
case accumulates into a non-zero dW, with and without the bias gradient."""
import functools

import pytest
import torch
import torch.nn.functional as F

from veles_amd import ops
from veles_amd.ops import _lib

pytestmark = pytest.mark.gpu

# (N, H, W, C, OC, K, pad, groups)
SHAPES = {
    "conv3": (2, 13, 13, 256, 384, 3, 1, 1),
    "conv3_n1": (1, 13, 13, 256, 384, 3, 1, 1),
    "conv5": (5, 13, 13, 384, 256, 3, 1, 2),
    "conv4": (3, 13, 13, 384, 384, 3, 1, 2),
    "conv2": (2, 27, 27, 96, 256, 5, 2, 2),
    "wide": (2, 20, 20, 128, 128, 3, 1, 1),
    "s2d55": (2, 57, 57, 48, 96, 3, 0, 1),
    "vgg56": (1, 56, 56, 128, 256, 3, 1, 1),
    "vgg112": (1, 112, 112, 64, 128, 3, 1, 1),
}
CASES = [(n, s) for n in SHAPES for s in (0, 7)]
# Steps per workgroup.  The launcher gives each of s splits ceil(steps / s)
# steps (the last split the rest).  conv3_n1: 169 pixels, three 64-pixel
# steps: 3 / 2 / 1 splits run 1 / 2 (and 1) / 3 steps.  s2d55: 2 images of
# 55 * 55 = 3025 pixels, 48 image-aligned steps each (the segment form counts
# steps): 96 / 48 / 32 splits run 1 / 2 / 3.  conv5: 5 * 169 = 845 pixels, 14
# steps in one workgroup per tile.
STEP_CASES = [("conv3_n1", 3, 1), ("conv3_n1", 2, 2), ("conv3_n1", 1, 3),
              ("s2d55", 96, 1), ("s2d55", 48, 2), ("s2d55", 32, 3),
              ("conv5", 1, 14)]


@functools.lru_cache(maxsize=None)
def _case(name):
    """Operands, the fp32 reference and the dW / db accumulated into, once
    per shape (read-only for the tests)."""
    N, H, W, C, OC, K, pad, groups = SHAPES[name]
    OH, OW = H + 2 * pad - K + 1, W + 2 * pad - K + 1
    g = torch.Generator(device="cuda").manual_seed(23)
    x = (torch.rand(N, H, W, C, generator=g, device="cuda") - 0.5).to(
        torch.bfloat16)
    dy = (torch.rand(N, OH, OW, OC, generator=g, device="cuda") - 0.5).to(
        torch.bfloat16)
    xp = F.pad(x.permute(0, 3, 1, 2).float(), (pad, pad, pad, pad))
    ref_w = torch.nn.grad.conv2d_weight(
        xp, (OC, C // groups, K, K), dy.permute(0, 3, 1, 2).float(),
        groups=groups).permute(0, 2, 3, 1).contiguous()
    ref_b = dy.float().reshape(-1, OC).sum(0)
    dw0 = torch.randn(OC, K, K, C // groups, generator=g, device="cuda")
    db0 = torch.randn(OC, generator=g, device="cuda")
    return x, dy, ref_w, ref_b, dw0, db0


def _geo(name, splits):
    N, H, W, C, OC, K, pad, groups = SHAPES[name]
    OH, OW = H + 2 * pad - K + 1, W + 2 * pad - K + 1
    return (N, H, W, C, OC, K, K, pad, pad, OH, OW, groups, splits)


def _halo(x, dy, dw, db, geo):
    fn = _lib.lib().hvk_conv_wgrad_halo
    stream = torch.cuda.current_stream().cuda_stream
    dbp = 0 if db is None else db.data_ptr()
    need = fn(x.data_ptr(), dy.data_ptr(), dw.data_ptr(), dbp, None, *geo,
              stream)
    assert need > 0, "shape does not take the halo kernel"
    ws = torch.empty(int(need), dtype=torch.float32, device="cuda")
    rc = fn(x.data_ptr(), dy.data_ptr(), dw.data_ptr(), dbp, ws.data_ptr(),
            *geo, stream)
    assert rc == 0
    torch.cuda.synchronize()


def _run(name, splits, bias, stages):
    x, dy, _, _, dw0, db0 = _case(name)
    dw = dw0.clone()
    db = db0.clone() if bias else None
    ops.set_halo_wgrad_stages(stages)
    try:
        _halo(x, dy, dw, db, _geo(name, splits))
    finally:
        ops.set_halo_wgrad_stages(True)
    return dw, db


def _check(name, splits, bias):
    x, dy, ref_w, ref_b, dw0, db0 = _case(name)
    OC = dy.shape[3]
    dw_one, db_one = _run(name, splits, bias, False)
    dw_two, db_two = _run(name, splits, bias, True)
    assert torch.equal(dw_two, dw_one)
    scale = ref_w.abs().max().item()
    err = (dw_two - dw0 - ref_w).abs().max().item()
    print("%s splits %d: err %.3e scale %.3e" % (name, splits, err, scale))
    assert err <= 2e-5 * max(scale, 1.0) * (dy.numel() / OC) ** 0.5, \
        (err, scale)
    if bias:
        assert torch.equal(db_two, db_one)
        berr = (db_two - db0 - ref_b).abs().max().item()
        assert berr <= 1e-3 * max(ref_b.abs().max().item(), 1.0), berr


@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("name,splits", CASES)
def test_two_stage_loop_equals_one_array_loop_and_fp32(name, splits, bias):
    _check(name, splits, bias)


@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("name,splits,steps", STEP_CASES)
def test_step_counts(name, splits, steps, bias):
    """1, 2 and 3 steps a workgroup (no pair, one pair, a pair and the tail
    step) and an even count over several image wraps."""
    N, H, W, C, OC, K, pad, groups = SHAPES[name]
    OH, OW = H + 2 * pad - K + 1, W + 2 * pad - K + 1
    seg = name == "s2d55"
    total = N * ((OH * OW + 63) // 64) if seg else (N * OH * OW + 63) // 64
    got = _lib.lib().hvk_conv_wgrad_halo_splits(*_geo(name, splits))
    assert got == splits, "the plan changed the split count"
    assert (total + splits - 1) // splits == steps
    _check(name, splits, bias)


def test_two_stage_loop_bit_stable():
    a, ab = _run("conv3", 0, True, True)
    b, bb = _run("conv3", 0, True, True)
    assert torch.equal(a, b) and torch.equal(ab, bb)
