"""Lean pixel loop of the halo weight gradient (csrc/kernels/wgrad_halo.hip,
LEAN; ops.set_halo_wgrad_lean) against the old loop, bit for bit, and
against the float32 PyTorch reference with test_wgrad_halo_gpu.py's bounds:
the full-row window with steps that straddle two images, a batch of one (no
second image), one workgroup walking several image wraps, MT 96, the 5 x 5
layer, the segment window (AlexNet conv1's space-to-depth image, VGG 56 and
112 wide); every case with the plan's own split and with seven ranges that
start mid-image and mid-row, accumulating into a non-zero dW, with and
without the bias gradient."""
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
# conv5 also as one workgroup per tile (14 steps over the five images)
CASES = [(n, s) for n in SHAPES
         for s in ((1, 0, 7) if n == "conv5" else (0, 7))]


@functools.lru_cache(maxsize=None)
def _case(name):
    """Operands, the fp32 reference and the dW / db accumulated into, once
    per shape (read-only for the tests)."""
    N, H, W, C, OC, K, pad, groups = SHAPES[name]
    OH, OW = H + 2 * pad - K + 1, W + 2 * pad - K + 1
    g = torch.Generator(device="cuda").manual_seed(11)
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


def _halo(x, dy, dw, db, K, pad, groups, splits):
    N, H, W, C = x.shape
    _, OH, OW, OC = dy.shape
    fn = _lib.lib().hvk_conv_wgrad_halo
    geo = (N, H, W, C, OC, K, K, pad, pad, OH, OW, groups, splits)
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


def _run(name, splits, bias, lean):
    x, dy, _, _, dw0, db0 = _case(name)
    _, _, _, _, _, K, pad, groups = SHAPES[name]
    dw = dw0.clone()
    db = db0.clone() if bias else None
    ops.set_halo_wgrad_lean(lean)
    try:
        _halo(x, dy, dw, db, K, pad, groups, splits)
    finally:
        ops.set_halo_wgrad_lean(True)
    return dw, db


@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("name,splits", CASES)
def test_lean_loop_equals_old_loop_and_fp32(name, splits, bias):
    x, dy, ref_w, ref_b, dw0, db0 = _case(name)
    OC = dy.shape[3]
    dw_old, db_old = _run(name, splits, bias, False)
    dw_lean, db_lean = _run(name, splits, bias, True)
    assert torch.equal(dw_lean, dw_old)
    scale = ref_w.abs().max().item()
    err = (dw_lean - dw0 - ref_w).abs().max().item()
    print("%s splits %d: err %.3e scale %.3e" % (name, splits, err, scale))
    assert err <= 2e-5 * max(scale, 1.0) * (dy.numel() / OC) ** 0.5, \
        (err, scale)
    if bias:
        assert torch.equal(db_lean, db_old)
        berr = (db_lean - db0 - ref_b).abs().max().item()
        assert berr <= 1e-3 * max(ref_b.abs().max().item(), 1.0), berr


def test_lean_loop_bit_stable():
    a, ab = _run("conv3", 0, True, True)
    b, bb = _run("conv3", 0, True, True)
    assert torch.equal(a, b) and torch.equal(ab, bb)
