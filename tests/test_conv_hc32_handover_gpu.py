"""conv_hc32's stage hand-over (csrc/kernels/conv_hc.hip, HO): the new order
(the stage barrier under the last k-step's MFMAs, the next stage's
bookkeeping in the k-loop's tail, the epilogue a compile-time choice) against
the round-6 order (ops.set_conv_hc32_handover(False)), bit for bit, and
against the float32 PyTorch reference on the same bf16 operands.

The persistent grid is capped (ops.set_conv_hc_max_wgs) at 1, 3 and 256
workgroups, so that these tiny shapes walk many items per workgroup: the
item-to-item hand-over (epilogue, new window, bias block, staged-store
barrier), the tile / n-tile / group changes inside one workgroup, and the
stage-to-stage hand-over of the shortest items (three stages)."""
import functools

import pytest
import torch
import torch.nn.functional as F

from veles_amd import ops

pytestmark = pytest.mark.gpu

CAPS = (1, 3, 256)

# name: kind, N, H, W, C, OC, K, pad, groups, activation, configuration
CASES = {
    # three pixel tiles (the last partial) x three n-tiles = 9 items
    "conv3_like": ("fwd", 7, 13, 13, 256, 384, 3, 1, 1, "str", 21),
    # group changes inside one workgroup
    "conv4_like": ("fwd", 7, 13, 13, 384, 384, 3, 1, 2, "str", 22),
    "ntile64": ("fwd", 7, 13, 13, 64, 64, 3, 1, 1, "str", 23),
    # 25 k-steps, three stages per item
    "conv2_like": ("fwd", 3, 27, 27, 96, 256, 5, 2, 2, "str", 24),
    # the conv1 shape after space-to-depth: 48 channels = three stages, the
    # bias block DMA'd two hand-overs before its epilogue
    "min_stages": ("fwd", 2, 15, 15, 48, 96, 3, 0, 1, "str", 22),
    "conv3_dgrad": ("dgrad", 7, 13, 13, 256, 384, 3, 1, 1, "str", 21),
    "conv5_dgrad": ("dgrad", 7, 13, 13, 384, 256, 3, 1, 2, "str", 22),
    # the generic (any activation, f32) epilogue
    "fwd_sigmoid": ("fwd", 7, 13, 13, 384, 384, 3, 1, 2, "sigmoid", 22),
    "dgrad_tanh": ("dgrad", 7, 13, 13, 384, 256, 3, 1, 2, "tanh", 22),
}

# (case, staged epilogue stores): backward-data runs with both
RUNS = [(name, ts) for name, c in CASES.items()
        for ts in ((1, 0) if c[0] == "dgrad" else (1,))]


def _r(*shape, scale=1.0, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return ((torch.rand(*shape, generator=g, device="cuda") - 0.5) *
            scale).to(torch.bfloat16)


def _close(a, b, tol):
    a, b = a.float(), b.float()
    err = (a - b).abs().max().item()
    assert err <= tol * (b.abs().max().item() + 1e-6), err


@functools.lru_cache(maxsize=None)
def _operands(name):
    """The case's operands and its float32 reference, computed once."""
    kind, N, H, W, C, OC, K, pad, g, act, _ = CASES[name]
    OH, OW = H + 2 * pad - K + 1, W + 2 * pad - K + 1
    x = _r(N, H, W, C, scale=2.0, seed=21)
    w = _r(OC, K, K, C // g, scale=0.2, seed=22)
    gb = torch.Generator(device="cuda").manual_seed(23)
    b = torch.randn(OC, device="cuda", generator=gb) * 0.1 + 0.05
    dy = _r(N, OH, OW, OC, scale=1.0, seed=24)
    if kind == "fwd":
        ref = F.conv2d(x.permute(0, 3, 1, 2).float(),
                       w.permute(0, 3, 1, 2).float(), b, padding=pad,
                       groups=g).permute(0, 2, 3, 1)
        ref = ref.clamp_min(0) if act == "str" else torch.sigmoid(ref)
    else:
        ref = torch.nn.grad.conv2d_input(
            (N, C, H, W), w.permute(0, 3, 1, 2).float(),
            dy.permute(0, 3, 1, 2).float(), padding=pad,
            groups=g).permute(0, 2, 3, 1)
        y = x.float()
        if act == "str":
            ref = ref * (y > 0)
        else:   # tanh through its output: 0.6666 * 1.7159 - 0.6666 / 1.7159 y^2
            ref = ref * (0.6666 * 1.7159 - (0.6666 / 1.7159) * y * y)
    return x, w, b, dy, ref.contiguous()


def _run(name, ts, cap, handover, times=1):
    kind, N, H, W, C, OC, K, pad, g, act, var = CASES[name]
    x, w, b, dy, _ = _operands(name)
    from veles_amd.ops import _lib
    lib = _lib.lib()
    prev = ops._CONV_HC
    outs = []
    try:
        ops.set_conv_hc(True, -1)
        ops.set_conv_hc32_handover(handover)
        ops.set_conv_hc_max_wgs(cap)
        lib.hvk_hc32_ts(ts)
        for _ in range(times):
            if kind == "fwd":
                outs.append(ops.conv_fwd(x, w, b, (1, 1), (pad,) * 4, g,
                                         act=act))
            else:
                outs.append(ops.conv_dgrad(dy, w, (N, H, W, C), (1, 1),
                                           (pad,) * 4, g, aux=x,
                                           aux_act=act))
        torch.cuda.synchronize()
        assert ops.conv_hc_last_variant() == var
    finally:
        lib.hvk_hc32_ts(1)
        ops.set_conv_hc_max_wgs(256)
        ops.set_conv_hc32_handover(True)
        ops.set_conv_hc(prev, -2)
    return outs


@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("name,ts", RUNS)
def test_handover_matches_round6_order_and_reference(name, ts, cap):
    new = _run(name, ts, cap, True)[0]
    old = _run(name, ts, cap, False)[0]
    assert torch.equal(new, old)
    _close(new, _operands(name)[4], 1e-2)


@pytest.mark.parametrize("name,ts", RUNS)
def test_handover_race_screen(name, ts):
    """20 runs at three workgroups: a sync-structure mistake shows as rare
    wrong tiles."""
    outs = _run(name, ts, 3, True, times=20)
    for o in outs[1:]:
        assert torch.equal(o, outs[0])
