"""Functional ops: hand-written HIP kernels on the GPU, PyTorch-fp32 references
on the CPU.

One code path for units: every op takes torch tensors; CUDA (HIP) tensors go
to ``libhvk.so`` (csrc/kernels, gfx950 MFMA / vectorised kernels) on the
current stream, CPU tensors are evaluated by the float32 reference below -
the numerics oracle of every kernel test (the reference's "numpy backend",
veles/backends.py:917-948).  There is no silent fallback: a GPU tensor with a
missing library raises ``KernelLibraryMissing``.

Layout conventions (docs/OPS.md): activations NHWC, conv weights
[OC][KH][KW][C/groups], fully-connected weights [out][in] (reference export
fixture libVeles/tests/workflow_files/contents.json), padding (left, top,
right, bottom), sliding (x, y).
"""
from __future__ import annotations

import math
import os
import struct

import torch
import torch.nn.functional as F

from veles_amd.ops import _lib
from veles_amd.ops._lib import available, require_library  # noqa: F401

__all__ = ["ACT", "gemm", "linear_fwd", "conv_out_size", "conv_fwd",
           "conv_dgrad", "conv_wgrad", "col_sum", "row_sum", "act_fwd",
           "act_bwd", "pool_fwd", "pool_bwd", "lrn_fwd", "lrn_bwd",
           "softmax_ce", "mse", "sgd_update", "dropout", "xorshift1024star",
           "xorshift128plus", "join", "cast", "fill_minibatch",
           "mean_disp_normalize", "act_code", "kohonen_coords",
           "kohonen_argmin", "kohonen_update", "lstm_fwd", "lstm_bwd",
           "rbm_layout", "rbm_uniforms", "rbm_sample", "rbm_grad",
           "bn_partials", "batchnorm_fwd", "batchnorm_bwd", "attention_fwd",
           "attention_bwd", "mha_fwd", "mha_bwd", "attn_head_dim",
           "ln_partials", "layernorm_fwd", "layernorm_bwd", "add",
           "FFN_ACT", "ffn_partials", "ffn_act_fwd", "ffn_act_bwd",
           "ffn_fwd", "ffn_bwd", "set_ffn_tile"]

DT = {torch.float32: 0, torch.bfloat16: 1, torch.uint8: 2, torch.int32: 3,
      torch.float16: 4}
ACT = {"linear": 0, None: 0, "tanh": 1, "relu": 2, "strict_relu": 3,
       "str": 3, "sigmoid": 4}


def act_code(act):
    if isinstance(act, int):
        return act
    return ACT[act]


def _p(t):
    return None if t is None else t.data_ptr()


def _s(t):
    return torch.cuda.current_stream(t.device).cuda_stream


def _lib_call(name, *args):
    fn = getattr(_lib.lib(), name)
    _lib.check(fn(*args), name)


def _gpu(t):
    return t is not None and t.is_cuda


# The LDS-DMA loaders address an operand through 32-bit buffer offsets
# (csrc/kernels/conv_geom.h kBufMaxBytes); a larger operand drops the kernel
# to its per-lane-address loader (VGG-16 b512 conv1_2: 3.3 GB activations,
# forward 3.1 ms on that path).  Convolutions over larger batches therefore
# run in image chunks that keep every operand under the limit.
_BUF_MAX = (1 << 31) - 64


def _image_chunks(N, *tensors):
    """Equal image ranges [(n0, n1)] whose slices of ``tensors`` (leading
    dimension = images) each stay under ``_BUF_MAX`` bytes."""
    per = max([t.numel() // max(t.shape[0], 1) * t.element_size()
               for t in tensors if t is not None] + [1])
    if N * per < _BUF_MAX or N < 2:
        return [(0, N)]
    n = max(1, (_BUF_MAX - 1) // per)
    k = -(-N // n)
    step = -(-N // k)
    return [(i, min(N, i + step)) for i in range(0, N, step)]


# --------------------------------------------------------------- activations
def act_fwd_ref(x, act):
    act = act_code(act)
    if act == 1:
        return 1.7159 * torch.tanh(0.6666 * x)
    if act == 2:
        return torch.where(x > 15, x, torch.log1p(torch.exp(x.clamp(max=15))))
    if act == 3:
        return torch.clamp(x, min=0)
    if act == 4:
        return torch.sigmoid(x)
    return x


def act_bwd_ref(y, act):
    act = act_code(act)
    if act == 1:
        return 0.6666 * 1.7159 - (0.6666 / 1.7159) * y * y
    if act == 2:
        return 1 - torch.exp(-y)
    if act == 3:
        return (y > 0).to(y.dtype)
    if act == 4:
        return y * (1 - y)
    return torch.ones_like(y)


def act_fwd(x, act, out=None):
    act = act_code(act)
    if _gpu(x):
        out = torch.empty_like(x) if out is None else out
        _lib_call("hvk_act_fwd", _p(x), DT[x.dtype], _p(out), DT[out.dtype],
                  x.numel(), act, _s(x))
        return out
    r = act_fwd_ref(x.float(), act).to(x.dtype)
    if out is None:
        return r
    out.copy_(r)
    return out


XACT = {"log": 1, "tanhlog": 2, "sincos": 3, "mul": 4}


def xact_ref(x, kind, p=0.0, bwd=False, err=None):
    """float32 reference of hvk_xact: activations whose derivative is a
    function of the input x (log = asinh, tanhlog, sincos, mul)."""
    kind = XACT.get(kind, kind)
    x = x.float()
    if kind == 1:
        d = torch.rsqrt(x * x + 1) if bwd else torch.log(
            x + torch.sqrt(x * x + 1))
    elif kind == 2:
        a = x.abs()
        t = torch.tanh(torch.tensor(0.6666 * p))
        edge, slope = 1.7159 * t, 1.7159 * 0.6666 * (1 - t * t)
        th = torch.tanh(0.6666 * x)
        if bwd:
            d = torch.where(a <= p, 1.7159 * 0.6666 * (1 - th * th),
                            slope * p / a.clamp(min=p))
        else:
            d = torch.where(a <= p, 1.7159 * th, torch.sign(x) * (
                edge + slope * p * torch.log(a.clamp(min=p) / p)))
    elif kind == 3:
        flat = x.reshape(x.shape[0] if x.dim() > 1 else 1, -1)
        odd = (torch.arange(flat.shape[1], device=x.device) % 2 == 1)
        if bwd:
            d = torch.where(odd, -torch.sin(flat), torch.cos(flat))
        else:
            d = torch.where(odd, torch.cos(flat), torch.sin(flat))
        d = d.view(x.shape)
    elif kind == 4:
        d = torch.full_like(x, p) if bwd else x * p
    else:
        raise ValueError("unknown activation %r" % kind)
    return err.float() * d if bwd else d


def xact(x, kind, p=0.0, out=None, err=None):
    """y = f(x) (err None) or y = err * f'(x) for the input-derivative
    activations (``XACT``); ``hvk_xact`` on the GPU."""
    kind = XACT.get(kind, kind)
    bwd = err is not None
    if out is None:
        out = torch.empty_like(err if bwd else x)
    if _gpu(x):
        rowlen = x[0].numel() if x.dim() > 1 else x.numel()
        _lib_call("hvk_xact", _p(x), DT[x.dtype], _p(err),
                  DT[err.dtype] if bwd else 0, _p(out), DT[out.dtype],
                  x.numel(), int(kind), float(p), max(1, int(rowlen)),
                  int(bwd), _s(x))
        return out
    out.copy_(xact_ref(x, kind, p, bwd, err).to(out.dtype))
    return out


def gather(x, idx, out=None):
    """out[i] = x.flat[idx.flat[i]] (int32 indices; negative -> 0)."""
    if out is None:
        out = torch.empty(idx.shape, dtype=x.dtype, device=x.device)
    if _gpu(x):
        _lib_call("hvk_gather", _p(x), DT[x.dtype], _p(idx), _p(out),
                  DT[out.dtype], idx.numel(), _s(x))
        return out
    i = idx.reshape(-1).long()
    v = x.reshape(-1)[i.clamp(min=0)]
    v = torch.where(i >= 0, v, torch.zeros_like(v))
    out.copy_(v.view(out.shape))
    return out


def act_bwd(dy, y, act, out=None):
    """dx = dy * f'(y) (derivative expressed through the output y)."""
    act = act_code(act)
    if _gpu(dy):
        out = torch.empty_like(dy) if out is None else out
        _lib_call("hvk_act_bwd", _p(dy), DT[dy.dtype], _p(y), DT[y.dtype],
                  _p(out), DT[out.dtype], dy.numel(), act, _s(dy))
        return out
    r = (dy.float() * act_bwd_ref(y.float(), act)).to(dy.dtype)
    if out is None:
        return r
    out.copy_(r)
    return out


# --------------------------------------------------------------------- GEMM
def gemm(a, b, *, trans_a=False, trans_b=False, out=None, out_dtype=None,
         alpha=1.0, beta=0.0, bias=None, bias_mode="col", act=0, aux=None,
         aux_act=0, accumulate=False, splits=1, bias_grad=None,
         precision_level=None):
    """out[M][N] = act(alpha*op(a)@op(b) + beta*out + bias) * f'_aux(aux).

    ``accumulate``: out (float32) += alpha*op(a)@op(b) (+bias) - split-K
    partial sums are reduced with float atomics on the GPU.
    ``bias_grad`` (float32 [M], accumulate only): += alpha * row sums of
    op(a), computed by the same kernel (a ones column appended to op(b)).
    ``accumulate="overwrite"``: out (and bias_grad) := the product instead
    of +=, written without reading out - a weight gradient that is the
    step's only contribution (no zeroing pass needed before it).

    float32 / float64 GPU operands run the exact-precision MFMA SGEMM /
    DGEMM (csrc/kernels/gemm_f32.hip; alpha / beta / accumulate only) with
    the reference's ``precision_level`` 0 (plain), 1 (Kahan) or 2 (TwoSum
    multi-partial); default ``root.common.engine.precision_level``.
    """
    M = a.shape[1] if trans_a else a.shape[0]
    K = a.shape[0] if trans_a else a.shape[1]
    N = b.shape[0] if trans_b else b.shape[1]
    Kb = b.shape[1] if trans_b else b.shape[0]
    if K != Kb:
        raise ValueError("gemm: inner dimensions differ (%d vs %d)" % (K, Kb))
    act = act_code(act)
    aux_act = act_code(aux_act)
    bm = {"col": 1, "row": 2}[bias_mode]
    dev = a.device
    if out is None:
        out_dtype = out_dtype or (torch.float32 if accumulate else a.dtype)
        out = (torch.zeros if accumulate else torch.empty)(
            M, N, dtype=out_dtype, device=dev)
    overwrite = accumulate == "overwrite"
    if _gpu(a) and a.dtype in (torch.float32, torch.float64):
        return _gemm_fx(a, b, trans_a, trans_b, out, M, N, K, alpha, beta,
                        accumulate and not overwrite, precision_level, bias,
                        act, aux, bias_grad)
    if _gpu(a):
        if a.dtype != torch.bfloat16 or b.dtype != torch.bfloat16:
            raise TypeError("GPU gemm operands must be bfloat16 (or float32 "
                            "/ float64 for the exact-precision GEMM)")
        for t in (a, b, out):
            if t.stride(-1) != 1:
                raise ValueError("gemm operands must be row-major")
        if accumulate and out.dtype != torch.float32:
            raise TypeError("accumulate requires a float32 output")
        res = out
        pad = None
        if not accumulate and beta == 0.0 and bias_grad is None:
            pad = _dma_padded(a, b, trans_a, trans_b, M, N, K, bias, aux,
                              bm)
        if pad is not None:
            # odd M / N / K: zero-padded operands take the LDS-DMA loaders
            a, b, Mp, Np, Kp = pad
            out = torch.empty(Mp, Np, dtype=out.dtype, device=dev)
            M, N, K = Mp, Np, Kp
        # rows off the 16-B grid would drop the whole GEMM to the per-element
        # loaders (3001^3: 76 vs ~800 TF): re-stride such operands first
        a, b = _row_aligned(a), _row_aligned(b)
        if not accumulate and beta == 0.0 and out.dim() == 2 and \
                (out.stride(0) % 8 or out.data_ptr() % 16):
            # and a write-only output into an aligned buffer (vector
            # epilogue stores), copied out after
            out = torch.empty(M, -(-N // 8) * 8, dtype=out.dtype,
                              device=dev)[:, :N]
        atomic = 2 if overwrite else (1 if accumulate else 0)
        if splits > 1 and not accumulate:
            raise ValueError("split-K requires accumulate=True")
        if deterministic():
            splits = 1
        elif accumulate and splits == 1:
            # a weight gradient with a handful of output tiles and a long K
            # (CIFAR quick fc2: 10 x 64 over a 4096 batch, ONE workgroup
            # for 0.27 ms): split K over f32 atomics; an overwrite is then a
            # zero fill + atomic accumulate
            sp = _wgrad_gemm_splits(M, N + (bias_grad is not None), K)
            if sp > 1:
                if overwrite:
                    out.zero_()
                    if bias_grad is not None:
                        bias_grad.zero_()
                atomic, splits = 1, sp
        if bias_grad is not None and (trans_b or not accumulate):
            raise ValueError("bias_grad needs accumulate=True, trans_b=False")
        sk = 0 if accumulate or beta != 0.0 else \
            _splitk_for(a, b, trans_a, trans_b, out, M, N, K, bias, aux)
        if sk > 1:
            # a persistent f32 workspace of sk slices per size: each K split
            # stores its partial product to its own slice, the finishing
            # pass sums them in order (no atomics, nothing to zero)
            ws = _workspace(("splitk_ws", M * N * sk), (M * N * sk,),
                            torch.float32, dev)
            _lib_call("hvk_gemm_splitk", int(trans_a), int(trans_b), M, N, K,
                      _p(a), a.stride(0), _p(b), b.stride(0), _p(out),
                      out.stride(0), int(out.dtype == torch.float32),
                      float(alpha), _p(bias), act, _p(aux),
                      0 if aux is None else aux.stride(0), aux_act, sk,
                      _p(ws), 1, _s(a))
        else:
            _lib_call("hvk_gemm", int(trans_a), int(trans_b), M, N, K, _p(a),
                      a.stride(0), _p(b), b.stride(0), _p(out),
                      out.stride(0), int(out.dtype == torch.float32), atomic,
                      float(alpha), float(beta), _p(bias), bm, act, _p(aux),
                      0 if aux is None else aux.stride(0), aux_act,
                      int(splits), _p(bias_grad), _s(a))
        if res is not out:
            res.copy_(out[:res.shape[0], :res.shape[1]])
        return res
    A = a.float().t() if trans_a else a.float()
    B = b.float().t() if trans_b else b.float()
    r = alpha * (A @ B)
    if bias is not None:
        r = r + (bias.float().view(1, -1) if bm == 1 else
                 bias.float().view(-1, 1))
    if overwrite:
        out.copy_(r.to(out.dtype))
        if bias_grad is not None:
            bias_grad.copy_(alpha * A.sum(1))
        return out
    if accumulate:
        out += r.to(out.dtype)
        if bias_grad is not None:
            bias_grad += alpha * A.sum(1)
        return out
    if beta != 0.0:
        r = r + beta * out.float()
    r = act_fwd_ref(r, act)
    if aux is not None:
        r = r * act_bwd_ref(aux.float(), aux_act)
    out.copy_(r.to(out.dtype))
    return out


_DMA_PAD_MIN = 1 << 24   # M*N*K above which padding pays for its copies

# Deterministic mode (engine.deterministic / VELES_AMD_DETERMINISTIC=1):
# no f32-atomic reductions in the gradient path - GEMM weight gradients
# and GEMM-path conv weight gradients unsplit (one tile sums its whole K),
# column sums through torch's fixed-order reduction; the halo weight
# gradient and the workspace split-K GEMM are deterministic already.
# Two runs of the same step are then bit-identical (exact-resume tests);
# it costs the split-K parallelism of small weight gradients.
_DETERMINISTIC = os.environ.get("VELES_AMD_DETERMINISTIC", "0") != "0"


def set_deterministic(on):
    global _DETERMINISTIC
    _DETERMINISTIC = bool(on)


def deterministic():
    from veles_amd.utils.config import root, get
    return _DETERMINISTIC or bool(get(root.common.engine.deterministic,
                                      False))


def _dma_padded(a, b, trans_a, trans_b, M, N, K, bias, aux, bias_mode=1):
    """Zero-padded copies of a large GEMM's operands when an odd dimension
    keeps them off the LDS-DMA loaders (a K-major operand needs K % 8 == 0,
    an MN-major one M / N % 8 == 0; csrc/kernels/gemm.hip ``dma_ok``): K
    pads with zeros (adds nothing), M / N pads are sliced off the output.
    None when nothing needs padding, the GEMM is small, or a bias / aux
    operand would have to be padded too."""
    r8 = lambda v: -(-v // 8) * 8  # noqa: E731
    ka, kb = not trans_a, bool(trans_b)
    Kp = r8(K) if (ka or kb) and K % 8 else K
    Mp = r8(M) if not ka and M % 8 else M
    Np = r8(N) if not kb and N % 8 else N
    if (Mp, Np, Kp) == (M, N, K) or M * N * K < _DMA_PAD_MIN:
        return None
    # a per-column (1) / per-row (2) bias would be read past its end
    if bias is not None and (Np != N if bias_mode == 1 else Mp != M):
        return None
    if aux is not None and (Mp, Np) != (M, N):
        return None

    def padded(t, rows, cols):
        if tuple(t.shape) == (rows, cols):
            return t
        z = torch.zeros(rows, cols, dtype=t.dtype, device=t.device)
        z[:t.shape[0], :t.shape[1]].copy_(t)
        return z
    a2 = padded(a, M, Kp) if ka else padded(a, Kp, Mp)
    b2 = padded(b, Np, Kp) if kb else padded(b, Kp, Np)
    return a2, b2, Mp, Np, Kp


def _row_aligned(t):
    """``t`` itself when its rows start on 16-B boundaries, else a copy in a
    buffer whose row pitch is padded to a multiple of 8 elements (the view
    keeps the logical shape; the LDS-DMA loaders never read the pad)."""
    if t.dim() != 2 or (t.stride(0) % 8 == 0 and t.data_ptr() % 16 == 0):
        return t
    R, C = t.shape
    buf = torch.empty(R, -(-C // 8) * 8, dtype=t.dtype, device=t.device)
    v = buf[:, :C]
    v.copy_(t)
    return v


_SPLITK_ENV = os.environ.get("HVK_SPLITK")


def _wgrad_gemm_splits(M, N, K):
    """K splits for an accumulating GEMM under 64 output tiles with K >= 2048
    (~256 workgroups, >= 256 of K each); 1 = leave it whole.  The large FC
    weight gradients (AlexNet fc6: 2304 tiles) keep their single-pass
    read-modify-write.  HVK_SPLITK=0 disables."""
    if _SPLITK_ENV == "0" or K < 2048:
        return 1
    tiles = -(-M // 128) * -(-N // 128)
    if tiles >= 64:
        return 1
    return max(1, min(-(-256 // tiles), K // 256))


def _splitk_aligned(N, out, bias, aux):
    """Operands hvk_gemm_splitk takes (16-B rows for the finishing pass)."""
    return not (N % 8 or out.stride(0) % 8 or out.data_ptr() % 16 or
                (bias is not None and bias.data_ptr() % 16) or
                (aux is not None and (aux.stride(0) % 8 or
                                      aux.data_ptr() % 16)))


def auto_splitk(M, N, K, out, bias=None, aux=None):
    """K splits for a GEMM whose 128 x 128 output tiles cannot fill the
    MI355X's 256 CUs twice over (the FC layers at batch 512): enough splits
    for ~512 workgroups, each keeping >= 1024 of K.  0 = no split (shape or
    alignment not taken by hvk_gemm_splitk).  HVK_SPLITK=0 disables."""
    if _SPLITK_ENV == "0":
        return 0
    tiles = -(-M // 128) * -(-N // 128)
    if tiles >= 256 or K < 2048 or not _splitk_aligned(N, out, bias, aux):
        return 0
    sk = min(-(-512 // tiles), K // 1024)
    return sk if sk > 1 else 0


# the autotuner's replay forces a split count (ops/autotune.py)
_splitk_forced = None


def _splitk_for(a, b, trans_a, trans_b, out, M, N, K, bias, aux):
    """auto_splitk, overridden per shape by the device tuning table."""
    if _splitk_forced is not None:
        return _splitk_forced if _splitk_aligned(N, out, bias, aux) else 0
    sk = auto_splitk(M, N, K, out, bias, aux)
    # the table may also split a GEMM with 256..511 tiles (one 128 x 128
    # tile per CU: AlexNet b1024 fc6 forward runs 2 splits 7 % faster,
    # profiles/splitk_sweep_fc_r3.log)
    if _SPLITK_ENV == "0" or -(-M // 128) * -(-N // 128) >= 512 or \
            K < 1024 or not _splitk_aligned(N, out, bias, aux):
        return sk
    from veles_amd.ops import autotune
    autotune.log_call("splitk", (M, N, K), {
        "a": tuple(a.shape), "b": tuple(b.shape), "out": tuple(out.shape),
        "trans_a": trans_a, "trans_b": trans_b, "default": sk})
    t = autotune.lookup("splitk", M, N, K)
    return sk if t is None else (t if t > 1 else 0)


def _precision_level(level):
    if level is not None:
        return int(level)
    from veles_amd.utils.config import root, get
    return int(get(root.common.engine.precision_level, 0))


def _gemm_fx(a, b, ta, tb, out, M, N, K, alpha, beta, accumulate, level,
             bias, act, aux, bias_grad):
    if bias is not None or act_code(act) or aux is not None or \
            bias_grad is not None:
        raise ValueError("the float32/float64 GEMM takes alpha/beta only")
    if b.dtype != a.dtype or out.dtype != a.dtype:
        raise TypeError("gemm: mixed %s / %s / %s operands" %
                        (a.dtype, b.dtype, out.dtype))
    for t in (a, b, out):
        # a single column has no inner stride to speak of: torch keeps
        # whatever the tensor it was viewed from had ([1][K].t() is [K][1]
        # with strides (1, K)); its row pitch stride(0) is still right
        if t.stride(-1) != 1 and t.shape[-1] != 1:
            raise ValueError("gemm operands must be row-major")
    name = "hvk_gemm_f32" if a.dtype == torch.float32 else "hvk_gemm_f64"
    _lib_call(name, int(ta), int(tb), M, N, K, _p(a), a.stride(0), _p(b),
              b.stride(0), _p(out), out.stride(0), float(alpha),
              1.0 if accumulate else float(beta), _precision_level(level),
              _s(a))
    return out


def linear_fwd(x, w, bias=None, act=0, out=None):
    """y[B][out] = act(x[B][in] @ w[out][in]^T + bias)."""
    return gemm(x, w, trans_b=True, bias=bias, act=act, out=out)


# --------------------------------------------------------------- convolution
def conv_out_size(h, w, kh, kw, sliding, padding):
    sx, sy = sliding
    pl, pt, pr, pb = padding
    return (h + pt + pb - kh) // sy + 1, (w + pl + pr - kw) // sx + 1


def _nchw(x):
    return x.permute(0, 3, 1, 2).float()


def _nhwc(x):
    return x.permute(0, 2, 3, 1)


_WS = {}


def _branch_key():
    """The branch stream's id while a fan-out branch runs (units._Branches):
    concurrent branches must not share scratch buffers."""
    from veles_amd.units import _Branches
    br = _Branches.current()
    return None if br is None else id(br[0])


def _workspace(key, shape, dtype, device, zero=False):
    bk = _branch_key()
    if bk is not None:
        key = (key, "branch", bk)
    t = _WS.get(key)
    if t is None or tuple(t.shape) != tuple(shape) or t.dtype != dtype or \
            t.device != device:
        t = (torch.zeros if zero else torch.empty)(shape, dtype=dtype,
                                                   device=device)
        _WS[key] = t
    return t


_GROWN = {}
_RETIRED = []


def _grow_ws(name, n, dtype, device):
    """A scratch buffer of at least n elements shared by every call with this
    name (per device and fan-out branch), grown geometrically.  A buffer it
    outgrows stays allocated: a HIP graph captured earlier may still write
    into it on replay."""
    key = (name, str(device), dtype, _branch_key())
    t = _GROWN.get(key)
    if t is None or t.numel() < n:
        if t is not None:
            _RETIRED.append(t)
        size = max(n, 0 if t is None else t.numel() * 3 // 2)
        t = _GROWN[key] = torch.empty(size, dtype=dtype, device=device)
    return t[:n]


def needs_im2col(C, groups):
    """Small-channel convs (C/groups % 8 != 0, e.g. RGB input) run as an
    explicit bf16 im2col + dense MFMA GEMM instead of per-element gathers."""
    return groups == 1 and C % 8 != 0


# Small-channel (3 <= C < 8, e.g. RGB at stride 1) convs: zero-pad the
# channels to 8 and run the implicit-GEMM path instead of the packed
# (kw, c)-run kernels.  VGG-16 conv1_1 (b128, 224^2): weight gradient 0.82 ->
# 0.32 ms (+0.05 ms for the pad, shared with the forward), forward 1.41 ->
# 1.26 ms (tools/bench_c3_pad.py).  HVK_C3_PAD=0 keeps the run kernels.
_C_PAD8 = os.environ.get("HVK_C3_PAD", "1") != "0"
_DIRECT = os.environ.get("HVK_CONV_DIRECT", "1") != "0"
_C_PAD_MIN = int(os.environ.get("HVK_C3_PAD_MIN", "3"))


def pad8_ok(C, groups):
    """Channels padded to the next multiple of 8 (3 -> 8, LeNet's 20 -> 24)."""
    return _C_PAD8 and groups == 1 and C >= _C_PAD_MIN and C % 8 != 0


def _cpad(C):
    return -(-C // 8) * 8


class PaddedImage(object):
    """The channel-padded image of a small-channel conv input, kept by the
    forward pass for the weight-gradient GEMM."""

    def __init__(self, x, C):
        self.x = x
        self.C = C


def _pad_channels(x):
    """x [N,H,W,C] -> [N,H,W,Cp] (Cp = C rounded up to 8), the padding
    channels zero (a persistent buffer per input tensor: the pad stays zero,
    only x's channels are copied)."""
    N, H, W, C = x.shape
    buf = _workspace(("cpad8", x.data_ptr(), N, H, W, C),
                     (N, H, W, _cpad(C)), x.dtype, x.device, zero=True)
    buf[..., :C].copy_(x)
    return buf


def _pad_weights(w, key):
    OC, KH, KW, C = w.shape
    wp = _workspace((key, id(w)), (OC, KH, KW, _cpad(C)), w.dtype,
                    w.device, zero=True)
    wp[..., :C].copy_(w)
    return wp


class S2DImage(object):
    """The space-to-depth image of a strided small-channel conv input: kept
    by the forward pass for the weight-gradient GEMM, or served directly by
    the loader's fused gather (``fill_minibatch_s2d``) as the conv input.
    ``shape`` is the NHWC shape of the image it stands for."""
    __slots__ = ("x", "s", "shape")

    def __init__(self, x, s, shape=None):
        self.x = x
        self.s = s
        self.shape = tuple(shape) if shape is not None else None


_S2D = os.environ.get("HVK_S2D", "1") != "0"   # A/B knob


def s2d_factor(C, groups, sliding, KH, KW):
    """Stride s when a conv is better run as space-to-depth (C -> s*s*C
    channels, stride 1, ceil(K/s) taps): small C, equal strides, s*s*C a
    multiple of 8 (the aligned LDS-DMA loaders), kernel at least s wide."""
    sx, sy = sliding
    if groups != 1 or C % 8 == 0 or sx != sy or sx < 2 or not _S2D:
        return 0
    if (sx * sx * C) % 8 or KH < sx or KW < sx:
        return 0
    return sx


def _s2d_geometry(H, W, KH, KW, s, padding):
    OH, OW = conv_out_size(H, W, KH, KW, (s, s), padding)
    KH2, KW2 = -(-KH // s), -(-KW // s)
    return OH, OW, KH2, KW2, OH - 1 + KH2, OW - 1 + KW2


def s2d_geometry(shape, s, KH, KW, padding):
    """(H2, W2, C2) of the space-to-depth image of an NHWC ``shape``."""
    _, H, W, C = shape
    _, _, _, _, H2, W2 = _s2d_geometry(H, W, KH, KW, s, padding)
    return H2, W2, s * s * C


def space_to_depth_ref(x, s, KH, KW, padding):
    """Torch reference of hvk_space_to_depth: x [N,H,W,C] ->
    [N,H2,W2,s*s*C], y[n,Y,X,dy,dx,c] = x[n, s*Y+dy-pt, s*X+dx-pl, c] (0
    outside the image)."""
    N, H, W, C = x.shape
    _, _, _, _, H2, W2 = _s2d_geometry(H, W, KH, KW, s, padding)
    pl, pt = padding[0], padding[1]
    xp = F.pad(x.permute(0, 3, 1, 2), (pl, s * W2 - W - pl, pt,
                                       s * H2 - H - pt))
    xp = xp.permute(0, 2, 3, 1)   # [N, s*H2, s*W2, C]
    return xp.reshape(N, H2, s, W2, s, C).permute(0, 1, 3, 2, 4, 5) \
        .reshape(N, H2, W2, s * s * C).contiguous()


def s2d_affine(vec, sample_shape, s, KH, KW, padding, fill):
    """A per-feature vector over an [H,W,C] sample laid out in space-to-depth
    order (``fill`` where the s2d image has no input pixel): the mean /
    rdisp of ``fill_minibatch_s2d``."""
    H, W, C = sample_shape
    y = space_to_depth_ref(vec.reshape(1, H, W, C).float(), s, KH, KW,
                           padding)
    if fill:   # exact values inside, ``fill`` where no input pixel is
        inb = space_to_depth_ref(torch.ones(1, H, W, C), s, KH, KW, padding)
        y = torch.where(inb > 0, y, torch.full_like(y, float(fill)))
    return y.reshape(-1).contiguous()


def fill_minibatch_s2d(src, shuffled, start, count, dst, s, KH, KW, padding,
                       mean2, rdisp2, labels=None, labels_out=None,
                       idx_out=None):
    """fill_minibatch fused with the first conv's space-to-depth transform:
    dst [n,H2,W2,s*s*C] = s2d((src[shuffled[start+i]] - mean) * rdisp),
    with ``mean2`` / ``rdisp2`` from ``s2d_affine``.  Same labels / indices
    outputs as fill_minibatch."""
    N, H, W, C = src.shape
    max_mb = dst.shape[0]
    H2, W2, C2 = s2d_geometry(src.shape, s, KH, KW, padding)
    if _gpu(dst):
        _lib_call("hvk_fill_minibatch_s2d", _p(src), src.numel(),
                  _p(shuffled), int(start), int(count), max_mb, H, W, C, s,
                  padding[1], padding[0], H2, W2, _p(mean2), _p(rdisp2),
                  _p(dst), _p(labels), _p(labels_out), _p(idx_out), _s(dst))
        return dst
    idx = shuffled[start:start + count].long()
    v = src.reshape(N, -1)[idx].float()
    v = space_to_depth_ref(v.reshape(-1, H, W, C), s, KH, KW, padding)
    v = (v.reshape(len(idx), -1) - mean2.reshape(1, -1)) * \
        rdisp2.reshape(1, -1)
    # no input pixel: 0 in the normalised image (the conv's zero padding)
    inb = space_to_depth_ref(torch.ones(1, H, W, C), s, KH, KW,
                             padding).reshape(1, -1)
    v = v * inb
    d = dst.view(max_mb, -1)
    d[:count] = v.to(dst.dtype)
    d[count:] = 0
    if labels_out is not None:
        labels_out[:count] = labels[idx] if labels is not None else -1
        labels_out[count:] = -1
    if idx_out is not None:
        idx_out[:count] = idx.to(idx_out.dtype)
        idx_out[count:] = -1
    return dst


def space_to_depth(x, s, KH, KW, padding):
    N, H, W, C = x.shape
    _, _, KH2, KW2, H2, W2 = _s2d_geometry(H, W, KH, KW, s, padding)
    y = torch.empty(N, H2, W2, s * s * C, dtype=x.dtype, device=x.device)
    _lib_call("hvk_space_to_depth", _p(x), _p(y), N, H, W, C, s, padding[1],
              padding[0], H2, W2, _s(x))
    return y


def _s2d_weights(w, s):
    """[OC][KH][KW][C] -> the space-to-depth weights [OC][KH2][KW2][s*s*C]
    (taps past KH / KW zero) in one kernel."""
    OC, KH, KW, C = w.shape
    KH2, KW2 = -(-KH // s), -(-KW // s)
    w2 = _workspace(("s2dw", id(w)), (OC, KH2, KW2, s * s * C), w.dtype,
                    w.device)
    if _gpu(w) and w.dtype == torch.bfloat16 and w.is_contiguous():
        _lib_call("hvk_s2d_weights", _p(w), _p(w2), OC, KH, KW, C, s, _s(w))
        return w2
    wp = torch.zeros(OC, KH2 * s, KW2 * s, C, dtype=w.dtype, device=w.device)
    wp[:, :KH, :KW].copy_(w)   # taps past KH/KW stay zero
    w2.copy_(wp.view(OC, KH2, s, KW2, s, C).permute(0, 1, 3, 2, 4, 5)
             .reshape(OC, KH2, KW2, s * s * C))
    return w2


def im2col(x, KH, KW, sliding, padding, out=None):
    N, H, W, C = x.shape
    sx, sy = sliding
    pl, pt, pr, pb = padding
    OH, OW = conv_out_size(H, W, KH, KW, sliding, padding)
    K = KH * KW * C
    Kp = (K + 7) // 8 * 8
    M = N * OH * OW
    if out is None:
        out = torch.empty(M, Kp, dtype=x.dtype, device=x.device)
    if _gpu(x):
        _lib_call("hvk_im2col", _p(x), _p(out), N, H, W, C, KH, KW, sy, sx,
                  pt, pl, OH, OW, Kp, _s(x))
        return out
    xp = F.pad(_nchw(x), (pl, pr, pt, pb))
    cols = F.unfold(xp, (KH, KW), stride=(sy, sx))  # [N, C*KH*KW, L]
    cols = cols.view(N, C, KH, KW, -1).permute(0, 4, 2, 3, 1).reshape(M, K)
    out.zero_()
    out[:, :K] = cols.to(out.dtype)
    return out


# stride-1 convolutions with the input tile held in LDS
# (csrc/kernels/conv_halo.hip); False (VELES_AMD_HALO=0) runs every conv on
# the implicit GEMM
_HALO = os.environ.get("VELES_AMD_HALO", "1") != "0"
# the backward-data halo kernel measured slower than the implicit GEMM on
# every AlexNet shape (profiles/r3_experiments.md §9): off unless asked for
_HALO_DGRAD = os.environ.get("VELES_AMD_HALO_DGRAD", "0") != "0"


# channel-chunked halo convs (csrc/kernels/conv_hc.hip): stride-1 3 x 3 and
# 5 x 5 forward / backward-data with a per-chunk input window shared by
# every tap; on by default for the shapes where it measured faster
# (conv_hc.hip hc_plan, profiles/r5/ab_conv_hc_*.log)
_CONV_HC = os.environ.get("VELES_AMD_CONV_HC", "1") != "0"


def set_conv_hc(on, variant=None):
    """A/B knob of the channel-chunked halo conv kernels; ``variant``: -2
    the automatic shape policy (default), -1 every supported shape, > 0 one
    forced configuration of conv_hc.hip's table."""
    global _CONV_HC
    _CONV_HC = bool(on)
    if variant is not None and _lib.available():
        _lib.lib().hvk_hc_variant(int(variant))


def _hc_wpack(dgrad, N, H, W, C, OC, KH, KW, pt, pl, OH, OW, groups, out,
              aux, device):
    """The stage-major filter-bank workspace a conv_hc32 launch packs its
    weights into (csrc/kernels/conv_hc.hip hc32_pack_kernel), or None when
    the call does not take conv_hc32.  One buffer per device and fan-out
    branch, shared by the layers: each launch packs right before its conv
    on the same stream."""
    al = out.data_ptr() % 16 == 0 and (aux is None or aux.data_ptr() % 16 == 0)
    need = int(_lib.lib().hvk_conv_hc_wpack_bytes(
        dgrad, N, H, W, C, OC, KH, KW, pt, pl, OH, OW, groups, int(al)))
    if need <= 0:
        return None
    return _grow_ws("hc32_wpack", need // 2, torch.bfloat16, device)


def set_conv_hc32(on):
    """A/B knob of conv_hc.hip's 32x32x16-MFMA configurations (one tap per
    k-step; default on): off leaves the 16x16x32 two-taps-per-step kernel."""
    if _lib.available():
        _lib.lib().hvk_hc32(int(bool(on)))


def set_conv_hc32_handover(on):
    """A/B knob of conv_hc32's stage hand-over (default on: the stage barrier
    under the last k-step's MFMAs, the next stage's bookkeeping in the
    k-loop's tail); off is the round-6 order.  Results are bit-identical."""
    if _lib.available():
        _lib.lib().hvk_hc32_handover(int(bool(on)))


def set_conv_hc_max_wgs(n=256):
    """Cap of the persistent conv_hc grids (default 256, one workgroup per
    CU); tests lower it so that tiny shapes walk many items per workgroup."""
    if _lib.available():
        _lib.lib().hvk_hc_max_wgs(int(n))


def conv_hc_last_variant():
    """conv_hc.hip configuration of the last halo conv launch (tests)."""
    return int(_lib.lib().hvk_hc_last_variant())


def set_conv_halo(on, dgrad=None):
    """Enable / disable the LDS-halo stride-1 conv kernels (A/B runs);
    ``dgrad`` sets the backward-data kernel separately (default: same as
    ``on`` when given, else unchanged)."""
    global _HALO, _HALO_DGRAD
    _HALO = bool(on)
    if dgrad is not None:
        _HALO_DGRAD = bool(dgrad)


def _conv_fwd_call(x, w, bias, out, N, H, W, C, OC, KH, KW, sy, sx, pt, pl,
                   OH, OW, groups, act, stream, q8=None):
    """``q8``: the kernel arguments of a fused fp8 copy of ``out``
    (``fp8._q8_args`` + history length) or None.  Returns whether the fp8
    copy was written (the fused epilogue needs aligned rows and bias)."""
    chunks = _image_chunks(N, x)
    if len(chunks) > 1:
        fused = True
        for n0, n1 in chunks:
            qc = None
            if q8 is not None:
                qc = list(q8)
                qc[0] += n0 * OH * OW * OC     # one byte per element
            fused = _conv_fwd_call(
                x[n0:n1], w, bias, out[n0:n1], n1 - n0, H, W, C, OC, KH, KW,
                sy, sx, pt, pl, OH, OW, groups, act, stream, q8=qc) and fused
        return fused
    sfx = "" if q8 is None else "_q8"
    extra = [] if q8 is None else list(q8)
    if _CONV_HC and q8 is None and sy == 1 and sx == 1 and \
            out.is_contiguous() and x.dtype == torch.bfloat16:
        wp = _hc_wpack(0, N, H, W, C, OC, KH, KW, pt, pl, OH, OW, groups,
                       out, None, x.device)
        rc = _lib.lib().hvk_conv_fwd_hc(
            _p(x), _p(w), _p(bias), _p(out), N, H, W, C, OC, KH, KW, pt, pl,
            OH, OW, groups, act, _p(wp), stream)
        if rc == 0:
            return False
        if rc != -2:
            _lib.check(rc, "hvk_conv_fwd_hc")
    if _HALO and sy == 1 and sx == 1 and out.is_contiguous():
        rc = getattr(_lib.lib(), "hvk_conv_fwd_halo" + sfx)(
            _p(x), _p(w), _p(bias), _p(out), N, H, W, C, OC, KH, KW, pt, pl,
            OH, OW, groups, act, *extra, stream)
        if rc == 0:
            return True
        if rc == -3 and q8 is not None:
            # the fused output needs the vector epilogue (aligned rows,
            # bias): unfused call, the caller quantizes separately
            return _conv_fwd_call(x, w, bias, out, N, H, W, C, OC, KH, KW,
                                  sy, sx, pt, pl, OH, OW, groups, act, stream)
        if rc != -2:
            _lib.check(rc, "hvk_conv_fwd_halo" + sfx)
    rc = getattr(_lib.lib(), "hvk_conv_fwd" + sfx)(
        _p(x), _p(w), _p(bias), _p(out), N, H, W, C, OC, KH, KW, sy, sx, pt,
        pl, OH, OW, groups, act, *extra, stream)
    if rc == -3 and q8 is not None:
        _conv_fwd_call(x, w, bias, out, N, H, W, C, OC, KH, KW, sy, sx, pt,
                       pl, OH, OW, groups, act, stream)
        return False
    _lib.check(rc, "hvk_conv_fwd" + sfx)
    return q8 is not None


def conv_fwd(x, w, bias=None, sliding=(1, 1), padding=(0, 0, 0, 0),
             groups=1, act=0, out=None, col_out=None, q8=None,
             q8_scaler=None):
    """x [N,H,W,C], w [OC,KH,KW,C/g] -> y [N,OH,OW,OC].

    ``col_out``: a dict that receives the im2col matrix when the explicit
    path is used (the weight-gradient GEMM reuses it).  ``q8`` /
    ``q8_scaler``: also write the fp8 copy of y that the fp8 layer reading
    it takes (``ops.fp8.conv_fwd`` semantics) - from the GEMM / halo
    epilogue where the kernel path has one, else by a separate quantize
    pass."""
    if q8 is None:
        return _conv_fwd(x, w, bias, sliding, padding, groups, act, out,
                         col_out, None)
    from veles_amd.ops import fp8
    if not _gpu(x):
        y = _conv_fwd(x, w, bias, sliding, padding, groups, act, out,
                      col_out, None)
        fp8._q8_ref(y, q8, q8_scaler)
        return y
    fq = [fp8._q8_args(q8, q8_scaler) + [fp8.HIST], False]
    y = _conv_fwd(x, w, bias, sliding, padding, groups, act, out, col_out,
                  fq)
    if not fq[1]:   # a kernel path without the fused output: separate pass
        fp8.quantize(y, q8_scaler, out=q8)
    return y


def _conv_fwd(x, w, bias, sliding, padding, groups, act, out, col_out, fq):
    """conv_fwd; ``fq`` = [q8 kernel arguments, fused flag] or None: the
    fused-epilogue calls pass the arguments and set the flag."""
    pre = x if isinstance(x, S2DImage) else None   # loader-made s2d input
    N, H, W, C = x.shape
    OC, KH, KW, Cg = w.shape
    if Cg * groups != C or OC % groups:
        raise ValueError("conv_fwd: bad grouping %s %s g=%d" %
                         (tuple(x.shape), tuple(w.shape), groups))
    sx, sy = sliding
    pl, pt, pr, pb = padding
    OH, OW = conv_out_size(H, W, KH, KW, sliding, padding)
    act = act_code(act)
    if pre is not None:
        if pre.s != s2d_factor(C, groups, sliding, KH, KW):
            raise ValueError("conv_fwd: s2d input of factor %d does not fit "
                             "this conv" % pre.s)
        x = pre.x
    if out is None:
        out = torch.empty(N, OH, OW, OC, dtype=x.dtype, device=x.device)
    elif tuple(out.shape) != (N, OH, OW, OC):
        raise ValueError("conv_fwd: out %s, expected %s" % (
            tuple(out.shape), (N, OH, OW, OC)))
    if _gpu(x):
        def call(*a):
            q = None
            if fq is not None and out.dtype == torch.bfloat16 and \
                    out.is_contiguous() and (OC // groups) % 8 == 0:
                q = fq[0]
            fused = _conv_fwd_call(*a, q8=q)
            if q is not None:
                fq[1] = fused
        s2 = s2d_factor(C, groups, sliding, KH, KW)
        if s2:
            # strided RGB conv as a stride-1 conv on the space-to-depth image
            _, _, KH2, KW2, H2, W2 = _s2d_geometry(H, W, KH, KW, s2, padding)
            x2 = pre.x if pre is not None else \
                space_to_depth(x, s2, KH, KW, padding)
            w2 = _s2d_weights(w, s2)
            C2 = s2 * s2 * C
            call(x2, w2, bias, out, N, H2, W2, C2, OC, KH2, KW2, 1, 1, 0, 0,
                 OH, OW, 1, act, _s(x))
            if col_out is not None:
                col_out["col"] = S2DImage(x2, s2, (N, H, W, C))
            return out
        if pad8_ok(C, groups):
            xp = _pad_channels(x)
            wp8 = _pad_weights(w, "wpad8")
            call(xp, wp8, bias, out, N, H, W, _cpad(C), OC, KH, KW, sy, sx,
                 pt, pl, OH, OW, 1, act, _s(x))
            if col_out is not None:
                col_out["col"] = PaddedImage(xp, C)
            return out
        if _DIRECT and groups == 1 and C < 3 and KH * KW * C <= 64 and \
                OC <= 64 and out.is_contiguous() and \
                _lib.lib().hvk_conv_fwd_direct(
                    _p(x), _p(w), _p(bias), _p(out), N, H, W, C, OC, KH, KW,
                    sy, sx, pt, pl, OH, OW, act, _s(x)) == 0:
            # a reduction this short (LeNet conv1: 25 taps) is latency bound
            # on the GEMM tile: direct per-pixel kernel
            return out
        if needs_im2col(C, groups):
            # packed (kw, c) runs: no im2col pass (csrc/kernels/gemm.hip)
            run = KW * C
            runp = (run + 7) // 8 * 8
            wp = _workspace(("wrun", id(w)), (OC, KH, runp), w.dtype,
                            w.device)
            if runp != run:
                wp[:, :, run:].zero_()
            wp[:, :, :run].copy_(w.reshape(OC, KH, run))
            _lib_call("hvk_conv_fwd_run", _p(x), _p(wp), _p(bias), _p(out),
                      N, H, W, C, OC, KH, KW, sy, sx, pt, pl, OH, OW, act,
                      _s(x))
            return out
        call(x, w, bias, out, N, H, W, C, OC, KH, KW, sy, sx, pt, pl, OH, OW,
             groups, act, _s(x))
        return out
    xp = F.pad(_nchw(x), (pl, pr, pt, pb))
    y = F.conv2d(xp, w.permute(0, 3, 1, 2).float(),
                 None if bias is None else bias.float(), stride=(sy, sx),
                 groups=groups)
    y = act_fwd_ref(y, act)
    out.copy_(_nhwc(y).to(out.dtype))
    return out


def _dgrad_hc_fwd_w(dy, w, out, aux, N, H, W, C, OC, KH, KW, sy, sx, pt, pl,
                    OH, OW, groups, aux_act):
    """Backward-data on conv_hc32 from the forward-layout weights: its
    filter-bank pack reads them directly, so the [g][c][kh][kw][oc]
    permutation pass is skipped.  False when that path does not apply (the
    caller permutes and dispatches as before)."""
    if not (_CONV_HC and sx == 1 and sy == 1 and out.is_contiguous() and
            dy.dtype == torch.bfloat16 and w.is_contiguous() and
            (aux is None or aux.is_contiguous())):
        return False
    chunks = list(_image_chunks(N, dy))
    if len(chunks) != 1:
        return False
    wp = _hc_wpack(1, N, H, W, C, OC, KH, KW, pt, pl, OH, OW, groups, out,
                   aux, dy.device)
    if wp is None:
        return False
    rc = _lib.lib().hvk_conv_dgrad_hc_w(
        _p(dy), _p(w), _p(out), N, H, W, C, OC, KH, KW, pt, pl, OH, OW,
        groups, _p(aux), aux_act, _p(wp), _s(dy))
    if rc in (-2, -3):
        return False
    _lib.check(rc, "hvk_conv_dgrad_hc_w")
    return True


def _dgrad_call(dy, wt, out, aux, N, H, W, C, OC, KH, KW, sy, sx, pt, pl,
                OH, OW, groups, aux_act):
    if _CONV_HC and sx == 1 and sy == 1 and out.is_contiguous() and \
            dy.dtype == torch.bfloat16 and \
            (aux is None or aux.is_contiguous()):
        wp = _hc_wpack(1, N, H, W, C, OC, KH, KW, pt, pl, OH, OW, groups,
                       out, aux, dy.device)
        rc = _lib.lib().hvk_conv_dgrad_hc(
            _p(dy), _p(wt), _p(out), N, H, W, C, OC, KH, KW, pt, pl, OH, OW,
            groups, _p(aux), aux_act, _p(wp), _s(dy))
        if rc == 0:
            return
        if rc != -2:
            _lib.check(rc, "hvk_conv_dgrad_hc")
    if _HALO_DGRAD and sx == 1 and sy == 1 and out.is_contiguous():
        rc = _lib.lib().hvk_conv_dgrad_halo(
            _p(dy), _p(wt), _p(out), N, H, W, C, OC, KH, KW, pt, pl, OH,
            OW, groups, _p(aux), aux_act, _s(dy))
        if rc == 0:
            return
        if rc != -2:
            _lib.check(rc, "hvk_conv_dgrad_halo")
    _lib_call("hvk_conv_dgrad_t", _p(dy), _p(wt), _p(out), N, H, W, C,
              OC, KH, KW, sy, sx, pt, pl, OH, OW, groups, _p(aux),
              aux_act, _s(dy))


def conv_dgrad(dy, w, x_shape, sliding=(1, 1), padding=(0, 0, 0, 0),
               groups=1, aux=None, aux_act=0, out=None):
    """dx [N,H,W,C] = conv^T(dy, w) [* f'(aux)]."""
    N, H, W, C = x_shape
    _, OH, OW, OC = dy.shape
    _, KH, KW, Cg = w.shape
    sx, sy = sliding
    pl, pt, pr, pb = padding
    aux_act = act_code(aux_act)
    # the kernels index dy, w, aux and out with this geometry: a mismatch
    # would read or write out of bounds on the device
    if (Cg * groups != C or OC % groups or dy.shape[0] != N or
            w.shape[0] != OC or
            (OH, OW) != conv_out_size(H, W, KH, KW, sliding, padding) or
            (out is not None and tuple(out.shape) != (N, H, W, C)) or
            (aux is not None and tuple(aux.shape) != (N, H, W, C))):
        raise ValueError(
            "conv_dgrad geometry: x %s, dy %s, w %s, sliding %s, padding %s, "
            "groups %d" % (tuple(x_shape), tuple(dy.shape), tuple(w.shape),
                           sliding, padding, groups))
    if out is None:
        out = torch.empty(N, H, W, C, dtype=dy.dtype, device=dy.device)
    if _gpu(dy):
        # weights permuted to [g][c][kh][kw][oc]: a dense K-major B operand
        OCg, Cg = OC // groups, C // groups
        if groups == 1 and OC % 8:
            # an output-channel count off the 16-byte grid (LeNet's 50)
            # would force the per-element A loader (5x slower): zero-pad
            # dy's and the weights' channel dimension to a multiple of 8
            OCp = -(-OC // 8) * 8
            wt = _workspace(("dgrad_wtp", id(w)), (1, C, KH, KW, OCp),
                            w.dtype, w.device, zero=True)
            wt[..., :OC].copy_(w.view(1, OC, KH, KW, C).permute(
                0, 4, 2, 3, 1))
            dyp = _workspace(("dgrad_dyp", N, OH, OW, OCp), (N, OH, OW, OCp),
                             dy.dtype, dy.device, zero=True)
            dyp[..., :OC].copy_(dy)
            dy, OC = dyp, OCp
        else:
            if _dgrad_hc_fwd_w(dy, w, out, aux, N, H, W, C, OC, KH, KW, sy,
                               sx, pt, pl, OH, OW, groups, aux_act):
                return out
            wt = _workspace(("dgrad_wt", id(w)), (groups, Cg, KH, KW, OCg),
                            w.dtype, w.device)
            wt.copy_(w.view(groups, OCg, KH, KW, Cg).permute(0, 4, 2, 3, 1))
        for n0, n1 in _image_chunks(N, dy):
            _dgrad_call(dy[n0:n1], wt, out[n0:n1],
                        None if aux is None else aux[n0:n1], n1 - n0, H, W,
                        C, OC, KH, KW, sy, sx, pt, pl, OH, OW, groups, aux_act)
        return out
    Hp, Wp = H + pt + pb, W + pl + pr
    dxp = torch.nn.grad.conv2d_input((N, C, Hp, Wp),
                                     w.permute(0, 3, 1, 2).float(),
                                     _nchw(dy), stride=(sy, sx), groups=groups)
    dx = dxp[:, :, pt:pt + H, pl:pl + W]
    if aux is not None:
        dx = dx * act_bwd_ref(_nchw(aux), aux_act)
    out.copy_(_nhwc(dx).to(out.dtype))
    return out


def conv_wgrad(x, dy, dw, sliding=(1, 1), padding=(0, 0, 0, 0), groups=1,
               splits=None, col=None, dbias=None):
    """dw (float32 [OC,KH,KW,C/g]) += sum over pixels of dy (x) im2col(x);
    ``dbias`` (float32 [OC]) += sum over pixels of dy, fused into the same
    GEMM.  ``col``: an explicit im2col matrix to use instead (optional)."""
    if isinstance(x, S2DImage):   # loader-made s2d input (conv_fwd)
        col, x = x, x.x
        N, H, W, C = col.shape
    else:
        N, H, W, C = x.shape
    _, OH, OW, OC = dy.shape
    _, KH, KW, Cg = dw.shape
    sx, sy = sliding
    pl, pt, pr, pb = padding
    if dw.dtype != torch.float32:
        raise TypeError("conv_wgrad accumulates into float32")
    # the kernels index x, dy and dw with this geometry: a mismatch would
    # read out of bounds on the device
    if (Cg * groups != C or OC % groups or dy.shape[0] != N or
            OH != (H + pt + pb - KH) // sy + 1 or
            OW != (W + pl + pr - KW) // sx + 1):
        raise ValueError(
            "conv_wgrad geometry: x %s, dy %s, dw %s, sliding %s, padding "
            "%s, groups %d" % ((N, H, W, C), tuple(dy.shape), tuple(dw.shape),
                               sliding, padding, groups))
    if _gpu(x):
        xt = col.x if isinstance(col, (S2DImage, PaddedImage)) else x
        chunks = _image_chunks(N, xt, dy)
        if len(chunks) > 1:
            # a sum over pixels: the image chunks accumulate into dw / dbias
            for n0, n1 in chunks:
                c = col
                if isinstance(col, S2DImage):
                    c = S2DImage(col.x[n0:n1], col.s, (n1 - n0,) +
                                 tuple(col.shape[1:]))
                elif isinstance(col, PaddedImage):
                    c = PaddedImage(col.x[n0:n1], col.C)
                elif col is not None:
                    c = col[n0 * OH * OW:n1 * OH * OW]
                if isinstance(col, S2DImage) and col.x is x:
                    xc = c            # the loader-made s2d input itself
                else:
                    xc = x[n0:n1]
                conv_wgrad(xc, dy[n0:n1], dw, sliding, padding, groups,
                           None, c, dbias)
            return dw
        s2 = s2d_factor(C, groups, sliding, KH, KW)
        if s2:
            x2 = col.x if isinstance(col, S2DImage) else \
                space_to_depth(x, s2, KH, KW, padding)
            H2, W2, C2 = x2.shape[1], x2.shape[2], x2.shape[3]
            KH2, KW2 = -(-KH // s2), -(-KW // s2)
            # self-clearing workspace: zeroed once, cleared again by the fold
            dw2 = _workspace(("s2dg", dw.data_ptr()), (OC, KH2, KW2, C2),
                             torch.float32, dw.device, zero=True)
            if not _halo_wgrad(x2, dy, dw2, dbias, N, H2, W2, C2, OC, KH2,
                               KW2, 0, 0, OH, OW, 1, splits):
                # logged with the logical image shape: the autotuner
                # replays the call on a plain image (the s2d data has C2
                # channels)
                sp = splits or _wgrad_splits_for(
                    (N, H, W, C), dy, dw, sliding, padding, groups,
                    (N * OH * OW, OC, KH2 * KW2 * C2 + 1, 1))
                _lib_call("hvk_conv_wgrad", _p(x2), _p(dy), _p(dw2), N, H2,
                          W2, C2, OC, KH2, KW2, 1, 1, 0, 0, OH, OW, 1,
                          int(sp), _p(dbias), _s(x))
            if dw.is_contiguous():
                _lib_call("hvk_s2d_grad_fold", _p(dw2), _p(dw), OC, KH, KW, C,
                          s2, 1, _s(x))
                return dw
            full = dw2.view(OC, KH2, KW2, s2, s2, C).permute(
                0, 1, 3, 2, 4, 5).reshape(OC, KH2 * s2, KW2 * s2, C)
            dw += full[:, :KH, :KW]
            dw2.zero_()
            return dw
        if pad8_ok(C, groups):
            xp = col.x if isinstance(col, PaddedImage) and \
                col.x.shape[:3] == x.shape[:3] else _pad_channels(x)
            # self-clearing padded gradient: zeroed once, cleared after the fold
            Cp = _cpad(C)
            dwp = _workspace(("wgpad8", dw.data_ptr()), (OC, KH, KW, Cp),
                             torch.float32, dw.device, zero=True)
            sp = splits or _wgrad_splits_for(
                xp, dy, dwp, sliding, padding, 1,
                (N * OH * OW, OC, KH * KW * Cp + 1, 1))
            _lib_call("hvk_conv_wgrad", _p(xp), _p(dy), _p(dwp), N, H, W, Cp,
                      OC, KH, KW, sy, sx, pt, pl, OH, OW, 1, int(sp),
                      _p(dbias), _s(x))
            dw += dwp[..., :C]
            dwp.zero_()
            return dw
        if isinstance(col, (S2DImage, PaddedImage)):
            col = None
        if col is not None:
            K = KH * KW * Cg
            M = N * OH * OW
            sp = splits or wgrad_splits(M, OC, K, 1)
            gemm(dy.reshape(M, OC), col[:, :K], trans_a=True,
                 out=dw.view(OC, K), accumulate=True, splits=sp,
                 bias_grad=dbias)
            return dw
        if needs_im2col(C, groups):
            runp = (KW * C + 7) // 8 * 8
            sp = splits or _wgrad_splits_for(
                x, dy, dw, sliding, padding, groups,
                (N * OH * OW, OC, KH * runp + 1, 1))
            _lib_call("hvk_conv_wgrad_run", _p(x), _p(dy), _p(dw), _p(dbias),
                      N, H, W, C, OC, KH, KW, sy, sx, pt, pl, OH, OW,
                      int(sp), _s(x))
            return dw
        if (sy, sx) == (1, 1) and _halo_wgrad(x, dy, dw, dbias, N, H, W, C,
                                               OC, KH, KW, pt, pl, OH, OW,
                                               groups, splits):
            return dw
        if splits is None:
            splits = _wgrad_splits_for(
                x, dy, dw, sliding, padding, groups,
                (N * OH * OW, OC // groups, KH * KW * Cg + 1, groups))
        _lib_call("hvk_conv_wgrad", _p(x), _p(dy), _p(dw), N, H, W, C, OC, KH,
                  KW, sy, sx, pt, pl, OH, OW, groups, int(splits), _p(dbias),
                  _s(x))
        return dw
    xp = F.pad(_nchw(x), (pl, pr, pt, pb))
    g = torch.nn.grad.conv2d_weight(xp, (OC, Cg, KH, KW), _nchw(dy),
                                    stride=(sy, sx), groups=groups)
    dw += g.permute(0, 2, 3, 1)
    if dbias is not None:
        dbias += dy.float().reshape(-1, OC).sum(0)
    return dw


_HALO_WGRAD = os.environ.get("VELES_AMD_HALO_WGRAD", "1") != "0"


def set_halo_wgrad(on):
    """A/B knob of the halo weight-gradient kernel (env
    VELES_AMD_HALO_WGRAD)."""
    global _HALO_WGRAD
    _HALO_WGRAD = bool(on)


def set_halo_wgrad_lean(on):
    """A/B knob of the bf16 halo weight gradient's lean pixel loop (default
    on: DMA offsets from lane invariants and carried scalars, no division
    per step); off is the loop as it was.  Results are bit-identical."""
    if _lib.available():
        _lib.lib().hvk_halo_lean(int(bool(on)))


def set_halo_wgrad_stages(on):
    """A/B knob of the lean loop's LDS stages (default on: one LDS object
    per stage, so that the next step's DMA stays in flight under this
    step's fragment reads and MFMAs); off is the lean loop with both stages
    in one array.  Results are bit-identical."""
    if _lib.available():
        _lib.lib().hvk_halo_stages(int(bool(on)))


def _halo_wgrad(x, dy, dw, dbias, N, H, W, C, OC, KH, KW, pt, pl, OH, OW,
                groups, splits=None):
    """Stride-1 weight gradient on the halo kernel (csrc/kernels/
    wgrad_halo.hip) when the shape takes it: the input window of each
    64-pixel step is staged once and read by every tap; split over pixels
    into workspace slices that a finishing pass adds into dw / dbias in
    split order (deterministic).  ``splits``: the caller's pixel split
    count (None: the kernel's plan).  False: the caller uses
    hvk_conv_wgrad."""
    # the LDS-DMA loads need 16-B aligned X / dY: refuse misaligned views
    # here (the launch would fail after a plan-only call that said yes)
    if not _HALO_WGRAD or x.dtype != torch.bfloat16 or \
            dy.dtype != torch.bfloat16 or not dw.is_contiguous() or \
            not x.is_contiguous() or not dy.is_contiguous() or \
            x.data_ptr() % 16 or dy.data_ptr() % 16:
        return False
    from veles_amd.ops import _lib
    fn = _lib.lib().hvk_conv_wgrad_halo
    geo = (N, H, W, C, OC, KH, KW, pt, pl, OH, OW, groups,
           int(splits) if splits else 0)
    need = fn(_p(x), _p(dy), _p(dw), _p(dbias), None, *geo, _s(x))
    if need < 0:
        return False
    ws = _grow_ws("wgrad_halo_ws", int(need), torch.float32, x.device)
    rc = fn(_p(x), _p(dy), _p(dw), _p(dbias), _p(ws), *geo, _s(x))
    _lib.check(int(rc), "hvk_conv_wgrad_halo")
    return True


# 512 blocks (2 per CU) measured best on AlexNet b512 (72.7k img/s vs 71.6k
# at 2048 and 69.0k at 4096: fewer splits = fewer f32 atomics)
_WGRAD_BLOCKS = int(os.environ.get("HVK_WGRAD_BLOCKS", "512"))


def _wgrad_splits_for(x, dy, dw, sliding, padding, groups, shape):
    """wgrad_splits, overridden per shape by the device tuning table (the
    call's geometry is logged for the autotuner, ops/autotune.py)."""
    from veles_amd.ops import autotune
    default = wgrad_splits(*shape)
    autotune.log_call("wgrad", shape, {
        "x": tuple(x if isinstance(x, tuple) else x.shape), "dy": tuple(dy.shape), "dw": tuple(dw.shape),
        "sliding": tuple(sliding), "padding": tuple(padding),
        "groups": groups, "default": default})
    t = autotune.lookup("wgrad", *shape)
    if deterministic():
        return 1
    return default if t is None else max(1, t)


def wgrad_splits(P, M, N, groups, target_blocks=None):
    """Pixel (K) splits of a weight-gradient GEMM: enough blocks to fill the
    256 CUs, few enough that the f32 atomic reduction stays small (1 in
    deterministic mode: no atomics)."""
    if deterministic():
        return 1
    target_blocks = target_blocks or _WGRAD_BLOCKS
    tiles = ((M + 127) // 128) * ((N + 127) // 128) * groups
    splits = max(1, min(target_blocks // max(tiles, 1), P // 256))
    return splits


# ------------------------------------------------------------- reductions
def col_sum(x2d, out=None, scale=1.0, accumulate=False):
    """out[c] (+)= scale * sum_r x[r][c]  (float32 out)."""
    R, C = x2d.shape
    if out is None:
        out = torch.zeros(C, dtype=torch.float32, device=x2d.device)
    elif not accumulate:
        out.zero_()
    if _gpu(x2d) and not deterministic():
        _lib_call("hvk_col_sum", _p(x2d), DT[x2d.dtype], R, C, _p(out),
                  float(scale), _s(x2d))
        return out
    out += scale * x2d.float().sum(0)
    return out


def transpose_colsum(x2d, out=None, colsum=None, accumulate=False, ws=None):
    """out[C][R] = x[R][C]^T (bf16) and colsum[c] (+)= sum_r x[r][c] (float32,
    summed per 64-row slab, then the slabs in order: deterministic).  One
    pass over x: the FC weight gradient's dY^T plus its bias gradient.
    GPU: R and C multiples of 64; ws, float32 of (R / 64) * C, is the slab
    workspace (allocated when None)."""
    R, C = x2d.shape
    if out is None:
        out = torch.empty(C, R, dtype=x2d.dtype, device=x2d.device)
    if _gpu(x2d):
        if x2d.dtype != torch.bfloat16 or R % 64 or C % 64 or \
                not x2d.is_contiguous() or not out.is_contiguous():
            raise ValueError("transpose_colsum: contiguous bf16 with R, C "
                             "multiples of 64")
        if ws is None:
            ws = torch.empty(R // 64 * C, dtype=torch.float32,
                             device=x2d.device)
        _lib_call("hvk_transpose_colsum", _p(x2d), R, C, _p(out),
                  _p(colsum) if colsum is not None else None,
                  int(bool(accumulate)), _p(ws), _s(x2d))
        return out
    out.copy_(x2d.t())
    if colsum is not None:
        sums = x2d.float().sum(0)
        if accumulate:
            colsum += sums
        else:
            colsum.copy_(sums)
    return out


def row_sum(x2d, out=None, scale=1.0):
    R, C = x2d.shape
    if out is None:
        out = torch.empty(R, dtype=torch.float32, device=x2d.device)
    if _gpu(x2d):
        _lib_call("hvk_row_sum", _p(x2d), DT[x2d.dtype], R, C, _p(out),
                  float(scale), _s(x2d))
        return out
    out.copy_(scale * x2d.float().sum(1))
    return out


# ----------------------------------------------------------------- pooling
POOL = {"max": 0, "avg": 1, "maxabs": 2}


def pool_out_size(h, w, ky, kx, sy, sx):
    """Znicz pooling geometry: partial windows at the far edge are kept
    (ceil), never a window that starts outside the input: with a stride
    above the kernel size the ceil alone would count one (12 rows, 3 / 4:
    a fourth window at row 12), so the count stops at the last start below
    the size, (h - 1) // sy + 1.  Unchanged wherever sy <= ky: the ceil's
    last start is then below h - ky + sy <= h."""
    def n(size, kernel, stride):
        if size <= kernel:
            return 1
        return min((size - kernel + stride - 1) // stride,
                   (size - 1) // stride) + 1
    return n(h, ky, sy), n(w, kx, sx)


def _pool_ref(x, ky, kx, sy, sx, mode, OH, OW):
    N, H, W, C = x.shape
    xf = x.float()
    neg = float("-inf")
    # (a stride above the kernel size can leave the last rows uncovered)
    Hp, Wp = max(H, (OH - 1) * sy + ky), max(W, (OW - 1) * sx + kx)
    pad = torch.full((N, Hp, Wp, C), float("nan"))
    pad[:, :H, :W, :] = xf
    idx = torch.arange(N * H * W * C).view(N, H, W, C)
    pidx = torch.full((N, Hp, Wp, C), -1, dtype=torch.long)
    pidx[:, :H, :W, :] = idx
    best = torch.full((N, OH, OW, C), neg)
    bkey = torch.full((N, OH, OW, C), neg)
    bidx = torch.full((N, OH, OW, C), -1, dtype=torch.long)
    s = torch.zeros(N, OH, OW, C)
    cnt = torch.zeros(N, OH, OW, C)
    for dy in range(ky):
        for dx in range(kx):
            v = pad[:, dy:dy + (OH - 1) * sy + 1:sy, dx:dx + (OW - 1) * sx + 1:sx, :]
            vi = pidx[:, dy:dy + (OH - 1) * sy + 1:sy, dx:dx + (OW - 1) * sx + 1:sx, :]
            valid = ~torch.isnan(v)
            if mode == 1:
                s += torch.where(valid, v, torch.zeros_like(v))
                cnt += valid.float()
            else:
                key = v.abs() if mode == 2 else v
                better = valid & ((bidx < 0) | (key > bkey))
                best = torch.where(better, v, best)
                bkey = torch.where(better, key, bkey)
                bidx = torch.where(better, vi, bidx)
    if mode == 1:
        return s / cnt.clamp(min=1), None
    return best, bidx.to(torch.int32)


def pool_fwd(x, ky, kx, sliding=None, mode="max", out=None, argmax=None):
    """NHWC pooling; returns (y, argmax) - argmax is the flat input index of
    the chosen element (None for avg)."""
    sx, sy = sliding or (kx, ky)
    N, H, W, C = x.shape
    OH, OW = pool_out_size(H, W, ky, kx, sy, sx)
    m = POOL[mode]
    if out is None:
        out = torch.empty(N, OH, OW, C, dtype=x.dtype, device=x.device)
    if m != 1 and argmax is None:
        argmax = torch.empty(N, OH, OW, C, dtype=torch.int32, device=x.device)
    if _gpu(x):
        _lib_call("hvk_pool_fwd", _p(x), _p(out), _p(argmax), N, H, W, C, OH,
                  OW, ky, kx, sy, sx, 0, 0, m, _s(x))
        return out, argmax
    y, idx = _pool_ref(x.cpu(), ky, kx, sy, sx, m, OH, OW)
    out.copy_(y.to(out.dtype))
    if idx is not None:
        argmax.copy_(idx)
    return out, argmax


def stochastic_pool_u(n, seed, device="cpu"):
    """The uniforms hvk_stochastic_pool draws: (hash32(o, seed) >> 8) / 2^24
    for output element o."""
    o = torch.arange(n, dtype=torch.int64, device=device)
    return (_hash32(o, int(seed) & 0xFFFFFFFF) >> 8).float() / 16777216.0


def stochastic_pool(x, ky, kx, sliding=None, use_abs=False, train=True,
                    seed=0, seed_dev=None, out=None, argmax=None):
    """Stochastic pooling (NHWC): train - draw a window element with
    probability max(x, 0) / sum (|x| for use_abs; uniform when the sum is 0);
    test - the probability-weighted average.  Returns (y, argmax) with the
    flat input offset of the drawn (most probable) element.  GPU:
    ``hvk_stochastic_pool`` with the seed in device memory (``seed_dev``,
    int32 [1]); the CPU reference draws the same uniforms."""
    sx, sy = sliding or (kx, ky)
    N, H, W, C = x.shape
    OH, OW = pool_out_size(H, W, ky, kx, sy, sx)
    if out is None:
        out = torch.empty(N, OH, OW, C, dtype=x.dtype, device=x.device)
    if argmax is None:
        argmax = torch.empty(N, OH, OW, C, dtype=torch.int32, device=x.device)
    if _gpu(x):
        if seed_dev is None:
            seed_dev = torch.tensor([int(seed) & 0x7FFFFFFF],
                                    dtype=torch.int32, device=x.device)
        _lib_call("hvk_stochastic_pool", _p(x), _p(out), _p(argmax), N, H, W,
                  C, OH, OW, ky, kx, sy, sx, int(bool(use_abs)),
                  int(bool(train)), _p(seed_dev), _s(x))
        return out, argmax
    if seed_dev is not None:
        seed = int(seed_dev.reshape(-1)[0]) & 0xFFFFFFFF
    xf = x.float().cpu()
    # (a stride above the kernel size can leave the last rows uncovered)
    Hp, Wp = max(H, (OH - 1) * sy + ky), max(W, (OW - 1) * sx + kx)
    pad = torch.zeros(N, Hp, Wp, C)
    pad[:, :H, :W] = xf
    ok = torch.zeros(N, Hp, Wp, C, dtype=torch.bool)
    ok[:, :H, :W] = True
    idx = torch.full((N, Hp, Wp, C), -1, dtype=torch.long)
    idx[:, :H, :W] = torch.arange(N * H * W * C).view(N, H, W, C)
    vals, oks, ids = [], [], []
    for dy in range(ky):
        for dx in range(kx):
            sl = (slice(None), slice(dy, dy + (OH - 1) * sy + 1, sy),
                  slice(dx, dx + (OW - 1) * sx + 1, sx))
            vals.append(pad[sl])
            oks.append(ok[sl])
            ids.append(idx[sl])
    w = [(v.abs() if use_abs else v.clamp(min=0)) * o
         for v, o in zip(vals, oks)]
    tot = torch.zeros_like(vals[0])
    cnt = torch.zeros_like(vals[0])
    for wi, o in zip(w, oks):  # sequential, as the kernel sums
        tot = tot + wi
        cnt = cnt + o.float()
    inv = torch.where(tot > 0, 1.0 / tot.clamp(min=1e-38),
                      torch.zeros_like(tot))
    uni = 1.0 / cnt
    prs = [torch.where(tot > 0, wi * inv, uni) * o for wi, o in zip(w, oks)]
    y = torch.zeros_like(tot)
    pick = torch.full(tot.shape, -1, dtype=torch.long)
    if train:
        u = stochastic_pool_u(tot.numel(), seed).view(tot.shape)
        cum = torch.zeros_like(tot)
        taken = torch.zeros(tot.shape, dtype=torch.bool)
        for v, pr, o, i in zip(vals, prs, oks, ids):
            cum = cum + pr
            hit = o & ~taken & (cum >= u)
            fall = o & ~taken & ~hit
            y = torch.where(hit | fall, v, y)
            pick = torch.where(hit | fall, i, pick)
            taken = taken | hit
    else:
        best = torch.full(tot.shape, -1.0)
        for v, pr, o, i in zip(vals, prs, oks, ids):
            y = y + pr * v
            better = o & (pr > best)
            best = torch.where(better, pr, best)
            pick = torch.where(better, i, pick)
    out.copy_(y.to(out.dtype))
    argmax.copy_(pick.to(torch.int32))
    return out, argmax


def pool_bwd(dy, argmax, x_shape, ky, kx, sliding=None, mode="max",
             aux=None, aux_act=0, out=None):
    sx, sy = sliding or (kx, ky)
    N, H, W, C = x_shape
    _, OH, OW, _ = dy.shape
    m = POOL[mode]
    aux_act = act_code(aux_act)
    if out is None:
        out = torch.empty(N, H, W, C, dtype=dy.dtype, device=dy.device)
    if _gpu(dy):
        _lib_call("hvk_pool_bwd", _p(dy), _p(argmax), _p(out), N, H, W, C, OH,
                  OW, ky, kx, sy, sx, 0, 0, m, _p(aux), aux_act, _s(dy))
        return out
    g = dy.float()
    dx = torch.zeros(N * H * W * C)
    if m == 1:
        dx = dx.view(N, H, W, C)
        cnt = torch.zeros(N, OH, OW, C)
        for oh in range(OH):
            h0, h1 = oh * sy, min(oh * sy + ky, H)
            for ow in range(OW):
                w0, w1 = ow * sx, min(ow * sx + kx, W)
                c = (h1 - h0) * (w1 - w0)
                dx[:, h0:h1, w0:w1, :] += (g[:, oh, ow, :] / c)[:, None, None, :]
    else:
        dx.index_add_(0, argmax.long().reshape(-1), g.reshape(-1))
        dx = dx.view(N, H, W, C)
    if aux is not None:
        dx = dx * act_bwd_ref(aux.float(), aux_act)
    out.copy_(dx.to(out.dtype))
    return out


def pool2_ok(x_shape, ky, kx, sliding):
    """Geometry of the argmax-free 2 x 2 / stride-2 pooling kernels."""
    if len(x_shape) != 4:
        return False
    N, H, W, C = x_shape
    return ky == 2 and kx == 2 and tuple(sliding) == (2, 2) and \
        C % 8 == 0 and H % 2 == 0 and W % 2 == 0


def _q8_pool_args(q8, qs):
    from veles_amd.ops import fp8 as _f8
    if q8 is None:
        return [None, None, None, 1.0, 0, _f8.HIST]
    return [q8.data_ptr(), qs.state.data_ptr(), qs.shard.data_ptr(),
            float(qs.fmax_eff), qs.fmt, _f8.HIST]


# The pooling and LRN-pool kernels index with 32-bit element offsets (they
# refuse tensors of 2^31 elements or more): larger batches run in image
# chunks (every image is independent in these ops; NHWC slices along N stay
# contiguous and 16-B aligned for C % 8 == 0)
_CHUNK_ELEMS = 1 << 31


def _n_chunks(N, per_image):
    """[(n0, n1)] image ranges of under _CHUNK_ELEMS elements each, or
    None when the whole batch fits."""
    if N * per_image < _CHUNK_ELEMS:
        return None
    step = max(1, (_CHUNK_ELEMS - 1) // max(per_image, 1))
    return [(n0, min(N, n0 + step)) for n0 in range(0, N, step)]


def _sl(t, n0, n1):
    return None if t is None else t[n0:n1]


def _q8_sliceable(q8, N):
    """a fused fp8 copy splits with its result (the kernels only take the
    max of |result| into the scaler's shards: atomics, so chunks add up)"""
    return q8 is None or (q8.dim() == 4 and q8.shape[0] == N and
                          q8.is_contiguous())


def pool2_fwd(x, mode="max", out=None, q8=None, q8_scaler=None):
    """2 x 2 / stride-2 NHWC pooling that writes no argmax: ``pool2_bwd``
    recomputes the window's choice from x.  ``q8`` / ``q8_scaler``: also the
    fp8 copy of the result for the next fp8 layer (fused quantisation)."""
    N, H, W, C = x.shape
    m = POOL[mode]
    if out is None:
        out = torch.empty(N, H // 2, W // 2, C, dtype=x.dtype,
                          device=x.device)
    if _gpu(x):
        ch = _n_chunks(N, H * W * C) if _q8_sliceable(q8, N) else None
        if ch:
            for n0, n1 in ch:
                pool2_fwd(x[n0:n1], mode, out=out[n0:n1],
                          q8=_sl(q8, n0, n1), q8_scaler=q8_scaler)
            return out
        _lib_call("hvk_pool2_fwd_q8", _p(x), _p(out), N, H, W, C, m,
                  *_q8_pool_args(q8, q8_scaler), _s(x))
        return out
    y, _ = pool_fwd(x, 2, 2, (2, 2), mode, out=out)
    if q8 is not None:
        from veles_amd.ops import fp8 as _f8
        _f8._q8_ref(y, q8, q8_scaler)
    return y


def pool2_bwd(x, dy, mode="max", aux=None, aux_act=0, out=None, q8=None,
              q8_scaler=None):
    N, H, W, C = x.shape
    m = POOL[mode]
    aux_act = act_code(aux_act)
    if out is None:
        out = torch.empty_like(x, dtype=dy.dtype)
    if _gpu(x):
        ch = _n_chunks(N, H * W * C) if _q8_sliceable(q8, N) else None
        if ch:
            for n0, n1 in ch:
                pool2_bwd(x[n0:n1], dy[n0:n1], mode, aux=_sl(aux, n0, n1),
                          aux_act=aux_act, out=out[n0:n1],
                          q8=_sl(q8, n0, n1), q8_scaler=q8_scaler)
            return out
        _lib_call("hvk_pool2_bwd_q8", _p(x), _p(dy), _p(out), N, H, W, C, m,
                  _p(aux), aux_act, *_q8_pool_args(q8, q8_scaler), _s(x))
        return out
    if q8 is not None:
        dx = pool2_bwd(x, dy, mode, aux=aux, aux_act=aux_act, out=out)
        from veles_amd.ops import fp8 as _f8
        _f8._q8_ref(dx, q8, q8_scaler)
        return dx
    am = None
    if m != 1:
        _, am = pool_fwd(x, 2, 2, (2, 2), mode)
    return pool_bwd(dy, am, (N, H, W, C), 2, 2, (2, 2), mode, aux=aux,
                    aux_act=aux_act, out=out)


# --------------------------------------------------------------------- LRN
def _lrn_ref(x, n, alpha, beta, k):
    x2 = x * x
    half = n // 2
    xp = F.pad(x2, (half, half))
    s = sum(xp[..., i:i + x.shape[-1]] for i in range(2 * half + 1))
    return x * torch.pow(k + alpha * s, -beta)


def lrn_fwd(x, n=5, alpha=1e-4, beta=0.75, k=2.0, out=None):
    """Across-channel LRN on NHWC: y = x (k + alpha sum x^2)^-beta."""
    C = x.shape[-1]
    P = x.numel() // C
    if out is None:
        out = torch.empty_like(x)
    if _gpu(x):
        _lib_call("hvk_lrn_fwd", _p(x), _p(out), P, C, n, float(alpha),
                  float(beta), float(k), _s(x))
        return out
    out.copy_(_lrn_ref(x.float(), n, alpha, beta, k).to(out.dtype))
    return out


def lrn_bwd(x, dy, n=5, alpha=1e-4, beta=0.75, k=2.0, aux=None, aux_act=0,
            out=None):
    C = x.shape[-1]
    P = x.numel() // C
    aux_act = act_code(aux_act)
    if out is None:
        out = torch.empty_like(dy)
    if _gpu(x):
        _lib_call("hvk_lrn_bwd", _p(x), _p(dy), _p(out), P, C, n, float(alpha),
                  float(beta), float(k), _p(aux), aux_act, _s(x))
        return out
    xf = x.float().detach().requires_grad_(True)
    y = _lrn_ref(xf, n, alpha, beta, k)
    y.backward(dy.float())
    dx = xf.grad
    if aux is not None:
        dx = dx * act_bwd_ref(aux.float(), aux_act)
    out.copy_(dx.to(out.dtype))
    return out


# ------------------------------------------------------ batch normalisation
BN_CPU_CHAIN = 64     # CPU path: float32 sums of 64 rows, then of those


def _bn_fn(name):
    fn = getattr(_lib.lib(), name, None)
    if fn is None:
        raise _lib.KernelLibraryMissing(
            "%s lacks %s - rebuild with python -m veles_amd.ops.build" %
            (_lib.LIB_PATH, name))
    return fn


def bn_partials(P, C, vec):
    """Partials per channel of the two-launch reductions of ``hvk_bn_stats``
    and ``hvk_bn_bwd`` over [P][C]: a function of the shape and the path
    (``vec``: 8 channels per lane) only, never of the device."""
    g = _bn_fn("hvk_bn_partials")(int(P), int(C), int(bool(vec)))
    if g < 1:
        raise ValueError("batchnorm: no grid for P = %d, C = %d, vec = %s" %
                         (P, C, vec))
    return g


def _bn_chain_sum(t):
    """[P][C] float32 -> [C]: chains of BN_CPU_CHAIN rows, then their sums
    (no float32 chain is longer than BN_CPU_CHAIN + P / BN_CPU_CHAIN + 1)"""
    P = t.shape[0]
    k = P // BN_CPU_CHAIN * BN_CPU_CHAIN
    parts = [t[:k].view(-1, BN_CPU_CHAIN, t.shape[1]).sum(1)] if k else []
    if k < P:
        parts.append(t[k:].sum(0, keepdim=True))
    return torch.cat(parts).sum(0)


def _bn_rows(name, what, t, like=None):
    """(P, C, pitch) of a tensor whose last axis is the channel axis: any
    contiguous shape, or a 2-D view with contiguous rows"""
    if not isinstance(t, torch.Tensor):
        raise TypeError("%s: %s must be a tensor, got %s" % (
            name, what, type(t).__name__))
    if t.dim() < 1 or t.numel() < 1:
        raise ValueError("%s: %s is empty" % (name, what))
    C = t.shape[-1]
    if t.is_contiguous():
        ld = C
    elif t.dim() == 2 and t.stride(1) == 1 and t.stride(0) >= C:
        ld = t.stride(0)
    else:
        raise ValueError("%s: %s must be contiguous, or 2-D with contiguous "
                         "rows (strides %s)" % (name, what, t.stride()))
    if t.numel() >= 1 << 31:
        raise ValueError("%s: %s has %d elements, the limit is 2^31 - 1" % (
            name, what, t.numel()))
    if like is not None:
        if tuple(t.shape) != tuple(like.shape):
            raise ValueError("%s: %s is %s, x is %s" % (
                name, what, tuple(t.shape), tuple(like.shape)))
        if t.dtype != like.dtype:
            raise TypeError("%s: %s is %s, x is %s" % (
                name, what, t.dtype, like.dtype))
        if t.device != like.device:
            raise ValueError("%s: %s is on %s, x on %s" % (
                name, what, t.device, like.device))
    return t.numel() // C, C, ld


def _bn_vecs(name, C, x, **vecs):
    for what, v in vecs.items():
        if not isinstance(v, torch.Tensor):
            raise TypeError("%s: %s must be a tensor, got %s" % (
                name, what, type(v).__name__))
        if v.dtype != torch.float32:
            raise TypeError("%s: %s must be float32, not %s" % (
                name, what, v.dtype))
        if tuple(v.shape) != (C,) or not v.is_contiguous():
            raise ValueError("%s: %s must be a contiguous [%d], got %s" % (
                name, what, C, tuple(v.shape)))
        if v.device != x.device:
            raise ValueError("%s: %s is on %s, x on %s" % (
                name, what, v.device, x.device))


def _bn_xdtype(name, x):
    want = torch.bfloat16 if _gpu(x) else torch.float32
    if x.dtype != want:
        raise TypeError("%s: x must be %s on %s, not %s" % (
            name, want, x.device.type, x.dtype))


def _bn_vec(C, *pairs):
    fn = _bn_fn("hvk_bn_vec")
    return C % 8 == 0 and all(
        t is None or fn(_p(t), int(ld), C) for t, ld in pairs)


def batchnorm_fwd(x, gamma, beta, running_mean, running_var, training=True,
                  eps=1e-5, momentum=0.1, act=0, save=None, out=None,
                  ws=None):
    """Batch normalisation over the last axis of ``x`` (every other axis is
    a row): ``torch.nn.BatchNorm2d`` / ``BatchNorm1d`` followed by one of
    this project's activations.

    ``training``: y = act(gamma (x - mean) invstd + beta) with the rows'
    mean and biased variance; ``running_mean`` / ``running_var`` move by
    ``momentum`` towards the mean and the unbiased variance; ``save`` gets
    ``mean``, ``invstd`` (float32 [C]) and ``table`` (float32 [2][C]: scale
    = gamma invstd, shift = beta - mean scale).  Otherwise the running
    statistics take the place of the rows' and stay as they are.

    GPU: bf16 ``x`` / ``out``, float32 everything else (``hvk_bn_stats`` or
    ``hvk_bn_fold``, then ``hvk_bn_apply``).  CPU: float32 throughout.  A
    caller that keeps ``save`` and ``ws`` (dicts) gets the same buffers at
    every call."""
    name = "batchnorm_fwd"
    P, C, ldx = _bn_rows(name, "x", x)
    _bn_xdtype(name, x)
    _bn_vecs(name, C, x, gamma=gamma, beta=beta, running_mean=running_mean,
             running_var=running_var)
    act = act_code(act)
    if not 0 <= act <= 4:
        raise ValueError("%s: unknown activation %r" % (name, act))
    if training and P < 2:
        raise ValueError("%s: training needs more than one value per "
                         "channel, got %d" % (name, P))
    if out is None:
        out = torch.empty(x.shape, dtype=x.dtype, device=x.device)
    _, _, ldy = _bn_rows(name, "out", out, like=x)
    save = {} if save is None else save
    ws = {} if ws is None else ws
    dev = x.device
    mean = _rec_buf(save, "mean", (C,), torch.float32, dev)
    invstd = _rec_buf(save, "invstd", (C,), torch.float32, dev)
    table = _rec_buf(save, "table", (2, C), torch.float32, dev)
    if _gpu(x):
        s = _s(x)
        if training:
            vec = _bn_vec(C, (x, ldx))
            G = bn_partials(P, C, vec)
            w = _rec_buf(ws, "stats", (2 * C * G,), torch.float32, dev)
            _lib.check(_bn_fn("hvk_bn_stats")(
                _p(x), ldx, P, C, int(vec), _p(gamma), _p(beta),
                _p(running_mean), _p(running_var), float(eps),
                float(momentum), _p(mean), _p(invstd), _p(table), _p(w), s),
                "hvk_bn_stats")
        else:
            _lib.check(_bn_fn("hvk_bn_fold")(
                _p(gamma), _p(beta), _p(running_mean), _p(running_var), C,
                float(eps), _p(table), s), "hvk_bn_fold")
        _lib.check(_bn_fn("hvk_bn_apply")(
            _p(x), ldx, _p(out), ldy, P, C, _p(table), act, s),
            "hvk_bn_apply")
        return out
    x2 = x.reshape(P, C)
    if training:
        m = _bn_chain_sum(x2) / P
        d = x2 - m
        var = _bn_chain_sum(d * d) / P
        mean.copy_(m)
        invstd.copy_(1.0 / torch.sqrt(var + eps))
        running_mean.mul_(1.0 - momentum).add_(momentum * m)
        running_var.mul_(1.0 - momentum).add_(
            momentum * (var * (P / (P - 1.0))))
        table[0].copy_(gamma * invstd)
        table[1].copy_(beta - m * table[0])
        y = d * table[0] + beta
    else:
        table[0].copy_(gamma / torch.sqrt(running_var + eps))
        table[1].copy_(beta - running_mean * table[0])
        y = (x2 - running_mean) * table[0] + beta
    out.copy_(act_fwd_ref(y, act).view(out.shape))
    return out


def batchnorm_bwd(err, x, y, gamma, save, dgamma, dbeta, act=0,
                  accumulate="overwrite", aux=None, aux_act=0, out=None,
                  ws=None, need_dx=True):
    """Backward of ``batchnorm_fwd(training=True)``.  g = err f'(y) when
    ``act`` is this layer's activation (0: ``y`` is not read and may be
    None); dbeta = sum g, dgamma = sum g xhat, written (``"overwrite"``) or
    added (True) to ``dbeta`` / ``dgamma``; returns dx = gamma invstd (g -
    dbeta / P - xhat dgamma / P), times f'(aux) of the layer below when
    ``aux_act`` is set (None with ``need_dx`` False).  ``save`` is the
    forward's.  GPU: ``hvk_bn_bwd`` (two reduction launches and the dx
    pass); CPU: float32."""
    name = "batchnorm_bwd"
    P, C, ldx = _bn_rows(name, "x", x)
    _bn_xdtype(name, x)
    _, _, lde = _bn_rows(name, "err", err, like=x)
    act, aux_act = act_code(act), act_code(aux_act)
    if not 0 <= act <= 4 or not 0 <= aux_act <= 4:
        raise ValueError("%s: unknown activation %r / %r" % (
            name, act, aux_act))
    if accumulate not in (True, "overwrite"):
        raise ValueError("%s: accumulate must be True or \"overwrite\"" %
                         name)
    ldy = lda = lddx = C
    if act:
        if y is None:
            raise ValueError("%s: the activation's derivative needs y" % name)
        _, _, ldy = _bn_rows(name, "y", y, like=x)
    else:
        y = None
    if aux_act:
        if aux is None:
            raise ValueError("%s: aux_act without aux" % name)
        _, _, lda = _bn_rows(name, "aux", aux, like=x)
    else:
        aux = None
    _bn_vecs(name, C, x, gamma=gamma, dgamma=dgamma, dbeta=dbeta)
    dev = x.device
    _rec_save_check(name, "batchnorm_fwd", save,
                    (("mean", (C,), torch.float32),
                     ("invstd", (C,), torch.float32)), dev)
    if P < 2:
        raise ValueError("%s: training needs more than one value per "
                         "channel, got %d" % (name, P))
    if need_dx:
        if out is None:
            out = torch.empty(x.shape, dtype=x.dtype, device=dev)
        _, _, lddx = _bn_rows(name, "out", out, like=x)
    else:
        out = None
    ws = {} if ws is None else ws
    mean, invstd = save["mean"], save["invstd"]
    if _gpu(x):
        vec = _bn_vec(C, (x, ldx), (err, lde), (y, ldy), (aux, lda),
                      (out, lddx))
        G = bn_partials(P, C, vec)
        w = _rec_buf(ws, "bwd", (2 * C * G,), torch.float32, dev)
        coef = _rec_buf(ws, "coef", (3, C), torch.float32, dev)
        _lib.check(_bn_fn("hvk_bn_bwd")(
            _p(x), ldx, _p(err), lde, _p(y), ldy, _p(aux), lda, _p(out),
            lddx, P, C, int(vec), _p(gamma), _p(mean), _p(invstd),
            _p(dgamma), _p(dbeta), int(accumulate is True), act, aux_act,
            _p(coef), _p(w), _s(x)), "hvk_bn_bwd")
        return out
    g = err.reshape(P, C)
    if act:
        g = g * act_bwd_ref(y.reshape(P, C), act)
    xh = (x.reshape(P, C) - mean) * invstd
    db = _bn_chain_sum(g)
    dg = _bn_chain_sum(g * xh)
    if accumulate is True:
        dbeta.add_(db)
        dgamma.add_(dg)
    else:
        dbeta.copy_(db)
        dgamma.copy_(dg)
    if out is None:
        return None
    dx = (gamma * invstd) * (g - db / P - xh * (dg / P))
    if aux_act:
        dx = dx * act_bwd_ref(aux.reshape(P, C), aux_act)
    out.copy_(dx.view(out.shape))
    return out


# ------------------------------- layer normalisation, residual connections
LN_CPU_CHAIN = 16     # CPU path: float32 sums of 16 columns, level by level


def ln_partials(P, C, vec):
    """Slices per column of the column sums (dgamma, dbeta) of
    ``hvk_ln_bwd`` over [P][C]: a function of the shape and the path
    (``vec``: 8 columns per lane) only, never of the device."""
    g = _bn_fn("hvk_ln_partials")(int(P), int(C), int(bool(vec)))
    if g < 1:
        raise ValueError("layernorm: no grid for P = %d, C = %d, vec = %s" %
                         (P, C, vec))
    return g


def _ln_row_sum(t):
    """[P][C] float32 -> [P]: sums of LN_CPU_CHAIN neighbours, level by
    level (no float32 chain is longer than LN_CPU_CHAIN per level)"""
    while t.shape[1] > 1:
        pad = -t.shape[1] % LN_CPU_CHAIN
        if pad:
            t = F.pad(t, (0, pad))
        t = t.reshape(t.shape[0], -1, LN_CPU_CHAIN).sum(2)
    return t[:, 0]


def _ln_vec(C, *pairs):
    fn = _bn_fn("hvk_ln_vec")
    return C % 8 == 0 and all(
        t is None or fn(_p(t), int(ld), C) for t, ld in pairs)


def layernorm_fwd(x, gamma, beta, *, residual=None, eps=1e-5, save=None,
                  out=None):
    """Layer normalisation over the last axis of ``x`` (every other axis is
    a row): ``torch.nn.LayerNorm(C, eps)`` of s = x (+ ``residual``):
    y = gamma (s - mean) invstd + beta with each row's mean and biased
    variance, in training and evaluation alike.  ``save`` gets ``mean`` and
    ``invstd`` (float32 [P]).  s is not stored: with a residual it is
    float(x) + float(residual) in float32, never rounded, and
    ``layernorm_bwd`` adds the two again.

    GPU: bf16 ``x`` / ``residual`` / ``out``, float32 everything else
    (``hvk_ln_fwd``, one launch).  CPU: float32 throughout.  A caller that
    keeps ``save`` (a dict) gets the same buffers at every call."""
    name = "layernorm_fwd"
    P, C, ldx = _bn_rows(name, "x", x)
    _bn_xdtype(name, x)
    _bn_vecs(name, C, x, gamma=gamma, beta=beta)
    ldr = C
    if residual is not None:
        _, _, ldr = _bn_rows(name, "residual", residual, like=x)
    if out is None:
        out = torch.empty(x.shape, dtype=x.dtype, device=x.device)
    _, _, ldy = _bn_rows(name, "out", out, like=x)
    save = {} if save is None else save
    dev = x.device
    mean = _rec_buf(save, "mean", (P,), torch.float32, dev)
    invstd = _rec_buf(save, "invstd", (P,), torch.float32, dev)
    if _gpu(x):
        _lib.check(_bn_fn("hvk_ln_fwd")(
            _p(x), ldx, _p(residual), ldr, _p(out), ldy, P, C, _p(gamma),
            _p(beta), float(eps), _p(mean), _p(invstd), _s(x)), "hvk_ln_fwd")
        return out
    s = x.reshape(P, C)
    if residual is not None:
        s = s + residual.reshape(P, C)
    m = _ln_row_sum(s) / C
    d = s - m[:, None]
    var = _ln_row_sum(d * d) / C
    mean.copy_(m)
    invstd.copy_(1.0 / torch.sqrt(var + eps))
    out.copy_(((d * invstd[:, None]) * gamma + beta).view(out.shape))
    return out


def layernorm_bwd(err, x, gamma, save, dgamma, dbeta, *, residual=None,
                  accumulate="overwrite", out=None, ws=None, need_dx=True):
    """Backward of ``layernorm_fwd``.  With sh = (s - mean) invstd and gh =
    err gamma: dbeta = sum_P err, dgamma = sum_P err sh, written
    (``"overwrite"``) or added (True) to ``dbeta`` / ``dgamma``; returns
    ds = invstd (gh - mean_C(gh) - sh mean_C(gh sh)) (None with ``need_dx``
    False), which is the gradient of x and of the residual alike.  ``save``
    is the forward's.  GPU: ``hvk_ln_bwd`` (the dx / column-partials launch
    or launches, then the finish); CPU: float32."""
    name = "layernorm_bwd"
    P, C, ldx = _bn_rows(name, "x", x)
    _bn_xdtype(name, x)
    _, _, lde = _bn_rows(name, "err", err, like=x)
    if accumulate not in (True, "overwrite"):
        raise ValueError("%s: accumulate must be True or \"overwrite\"" %
                         name)
    ldr = lddx = C
    if residual is not None:
        _, _, ldr = _bn_rows(name, "residual", residual, like=x)
    _bn_vecs(name, C, x, gamma=gamma, dgamma=dgamma, dbeta=dbeta)
    dev = x.device
    _rec_save_check(name, "layernorm_fwd", save,
                    (("mean", (P,), torch.float32),
                     ("invstd", (P,), torch.float32)), dev)
    if need_dx:
        if out is None:
            out = torch.empty(x.shape, dtype=x.dtype, device=dev)
        _, _, lddx = _bn_rows(name, "out", out, like=x)
    else:
        out = None
    ws = {} if ws is None else ws
    mean, invstd = save["mean"], save["invstd"]
    if _gpu(x):
        vec = _ln_vec(C, (err, lde), (x, ldx), (residual, ldr), (out, lddx),
                      (gamma, 8))
        G = ln_partials(P, C, vec)
        w = _rec_buf(ws, "bwd", (2 * C * G,), torch.float32, dev)
        _lib.check(_bn_fn("hvk_ln_bwd")(
            _p(err), lde, _p(x), ldx, _p(residual), ldr, _p(out), lddx, P, C,
            int(vec), _p(gamma), _p(mean), _p(invstd), _p(dgamma),
            _p(dbeta), int(accumulate is True), int(bool(need_dx)), _p(w),
            _s(x)), "hvk_ln_bwd")
        return out
    s = x.reshape(P, C)
    if residual is not None:
        s = s + residual.reshape(P, C)
    g = err.reshape(P, C)
    sh = (s - mean[:, None]) * invstd[:, None]
    db = _bn_chain_sum(g)
    dg = _bn_chain_sum(g * sh)
    if accumulate is True:
        dbeta.add_(db)
        dgamma.add_(dg)
    else:
        dbeta.copy_(db)
        dgamma.copy_(dg)
    if out is None:
        return None
    gh = g * gamma
    c1 = _ln_row_sum(gh) / C
    c2 = _ln_row_sum(gh * sh) / C
    out.copy_((invstd[:, None] * (gh - c1[:, None] - sh * c2[:, None]))
              .view(out.shape))
    return out


def add(a, b, out=None):
    """out = a + b over tensors of one shape whose last axis has contiguous
    elements (the residual add and the gradient fan-in).  GPU: bf16,
    ``hvk_add``: bf16(float(a) + float(b)); CPU: float32."""
    name = "add"
    P, C, lda = _bn_rows(name, "a", a)
    _bn_xdtype(name, a)
    _, _, ldb = _bn_rows(name, "b", b, like=a)
    if out is None:
        out = torch.empty(a.shape, dtype=a.dtype, device=a.device)
    _, _, ldo = _bn_rows(name, "out", out, like=a)
    if _gpu(a):
        _lib.check(_bn_fn("hvk_add")(
            _p(a), lda, _p(b), ldb, _p(out), ldo, P, C, _s(a)), "hvk_add")
        return out
    torch.add(a, b, out=out)
    return out


# ------------------------------------------------------- fused LRN -> pool
def lrn_pool_fusable(C, n, ky, kx, sliding):
    """Shapes the fused LRN -> 3x3 max-pool kernels take."""
    sx, sy = sliding
    return C % 8 == 0 and n // 2 <= 4 and ky == 3 and kx == 3 and \
        sx >= 2 and sy >= 2


def window_index_to_offsets(am, x_shape, ky, kx, sliding):
    """A uint8 window-local argmax (0 .. ky*kx-1, row-major inside the pooling
    window) -> flat int32 offsets into the NHWC input, the format of
    ``pool_fwd``'s argmax (reference paths and tests)."""
    sx, sy = sliding
    N, H, W, C = x_shape
    _, OH, OW, _ = am.shape
    dev = am.device
    a = am.long()
    oh = torch.arange(OH, device=dev).view(1, OH, 1, 1)
    ow = torch.arange(OW, device=dev).view(1, 1, OW, 1)
    n = torch.arange(N, device=dev).view(N, 1, 1, 1)
    c = torch.arange(C, device=dev).view(1, 1, 1, C)
    h = oh * sy + a // kx
    w = ow * sx + a % kx
    return (((n * H + h) * W + w) * C + c).to(torch.int32)


def lrn_pool_fwd(x, n, alpha, beta, k, ky, kx, sliding, out=None,
                 argmax=None):
    """max_pool(lrn(x)) without materialising lrn(x); ``argmax`` indexes the
    (virtual) LRN output, i.e. x's geometry.  A uint8 ``argmax`` (GPU,
    stride 2) holds the window-local index instead: 1 byte per element
    (``window_index_to_offsets`` converts)."""
    sx, sy = sliding
    N, H, W, C = x.shape
    OH, OW = pool_out_size(H, W, ky, kx, sy, sx)
    if out is None:
        out = torch.empty(N, OH, OW, C, dtype=x.dtype, device=x.device)
    if argmax is None:
        argmax = torch.empty(N, OH, OW, C, dtype=torch.int32, device=x.device)
    if _gpu(x):
        ch = _n_chunks(N, H * W * C) if argmax.dtype == torch.uint8 else None
        if ch:
            for n0, n1 in ch:
                lrn_pool_fwd(x[n0:n1], n, alpha, beta, k, ky, kx, sliding,
                             out=out[n0:n1], argmax=argmax[n0:n1])
            return out, argmax
        if argmax.dtype == torch.uint8:
            if (sx, sy) != (2, 2):
                raise ValueError("uint8 window-index argmax: stride 2 only")
            _lib_call("hvk_lrn_pool_fwd_u8", _p(x), _p(out), _p(argmax), N,
                      H, W, C, OH, OW, n, float(alpha), float(beta), float(k),
                      _s(x))
            return out, argmax
        _lib_call("hvk_lrn_pool_fwd", _p(x), _p(out), _p(argmax), N, H, W, C,
                  OH, OW, sy, sx, n, float(alpha), float(beta), float(k),
                  _s(x))
        return out, argmax
    y = lrn_fwd(x.float(), n, alpha, beta, k)
    if argmax.dtype == torch.uint8:
        yo, off = pool_fwd(y, ky, kx, sliding, "max", out=out)
        # window-local index of the chosen flat offset
        hw = (off.long() // C)
        h, w = (hw // W) % H, hw % W
        oh = torch.arange(OH).view(1, OH, 1, 1)
        ow = torch.arange(OW).view(1, 1, OW, 1)
        argmax.copy_(((h - oh * sy) * kx + (w - ow * sx)).to(torch.uint8))
        return yo, argmax
    return pool_fwd(y, ky, kx, sliding, "max", out=out, argmax=argmax)


def lrn_pool_bwd(x, dp, argmax, n, alpha, beta, k, ky, kx, sliding,
                 aux=None, aux_act=0, out=None):
    """lrn_bwd(x, pool_bwd(dp)) [* f'(aux)] without materialising the pool
    gradient."""
    sx, sy = sliding
    N, H, W, C = x.shape
    _, OH, OW, _ = dp.shape
    aux_act = act_code(aux_act)
    if out is None:
        out = torch.empty_like(x)
    if _gpu(x):
        ch = _n_chunks(N, H * W * C) if argmax.dtype == torch.uint8 else None
        if ch:
            for n0, n1 in ch:
                lrn_pool_bwd(x[n0:n1], dp[n0:n1], argmax[n0:n1], n, alpha,
                             beta, k, ky, kx, sliding, aux=_sl(aux, n0, n1),
                             aux_act=aux_act, out=out[n0:n1])
            return out
        if argmax.dtype == torch.uint8:
            _lib_call("hvk_lrn_pool_bwd_u8", _p(x), _p(dp), _p(argmax),
                      _p(out), N, H, W, C, OH, OW, n, float(alpha),
                      float(beta), float(k), _p(aux), aux_act, _s(x))
            return out
        _lib_call("hvk_lrn_pool_bwd", _p(x), _p(dp), _p(argmax), _p(out), N,
                  H, W, C, OH, OW, sy, sx, n, float(alpha), float(beta),
                  float(k), _p(aux), aux_act, _s(x))
        return out
    if argmax.dtype == torch.uint8:
        argmax = window_index_to_offsets(argmax, tuple(x.shape), ky, kx,
                                         sliding)
    g = pool_bwd(dp.float(), argmax, tuple(x.shape), ky, kx, sliding, "max")
    return lrn_bwd(x, g, n, alpha, beta, k, aux=aux, aux_act=aux_act,
                   out=out)


# --------------------------------------------------------------- evaluators
def softmax_ce(logits, labels, *, scale=None, err=None, probs=None,
               max_idx=None, metrics=None, confusion=None):
    """Fused softmax + cross-entropy gradient + error counting.

    err = (softmax(logits) - onehot(labels)) * scale (rows with label < 0 get
    0); metrics (float32[3]) += [n_err, sum CE loss, n_valid]."""
    B, C = logits.shape
    if scale is None:
        scale = 1.0 / B
    if _gpu(logits):
        _lib_call("hvk_softmax_ce", _p(logits), DT[logits.dtype], B, C,
                  _p(labels), float(scale), _p(err),
                  0 if err is None else DT[err.dtype], _p(probs), _p(max_idx),
                  _p(metrics), _p(confusion), _s(logits))
        return err
    lf = logits.float()
    p = torch.softmax(lf, 1)
    lab = labels.long() if labels is not None else torch.full(
        (B,), -1, dtype=torch.long)
    valid = lab >= 0
    if probs is not None:
        probs.copy_(p)
    if max_idx is not None:
        max_idx.copy_(lf.argmax(1).to(max_idx.dtype))
    if err is not None:
        oh = torch.zeros_like(p)
        oh[valid, lab[valid]] = 1.0
        e = (p - oh) * scale
        e[~valid] = 0
        err.copy_(e.to(err.dtype))
    if metrics is not None and valid.any():
        am = lf.argmax(1)
        pl = p[valid, lab[valid]].clamp(min=1e-30)
        metrics[0] += (am[valid] != lab[valid]).sum().float()
        metrics[1] += -torch.log(pl).sum()
        metrics[2] += valid.sum().float()
        if confusion is not None:
            for a, b in zip(am[valid].tolist(), lab[valid].tolist()):
                confusion[a, b] += 1
    return err


def mse(y, target, *, scale=1.0, err=None, mse_out=None, metrics=None,
        valid_rows=None):
    B = y.shape[0]
    D = y.numel() // B
    valid_rows = B if valid_rows is None else valid_rows
    if _gpu(y):
        _lib_call("hvk_mse", _p(y), DT[y.dtype], _p(target), DT[target.dtype],
                  B, D, float(scale), _p(err),
                  0 if err is None else DT[err.dtype], _p(mse_out),
                  _p(metrics), int(valid_rows), _s(y))
        return err
    d = y.float().reshape(B, D) - target.float().reshape(B, D)
    d[valid_rows:] = 0
    if err is not None:
        err.copy_((d * scale).reshape(err.shape).to(err.dtype))
    m = (d * d).mean(1)
    if mse_out is not None:
        mse_out.copy_(m)
    if metrics is not None:
        metrics[0] += m[:valid_rows].sum()
        metrics[1] += m[:valid_rows].sqrt().sum()
        metrics[2] += valid_rows
    return err


# --------------------------------------------------------------- optimizer
_SEG_CACHE = {}
_SEG_CACHE_MAX = 64


def _pack_sgd_segs(segs):
    return b"".join(struct.pack("<qqffff", int(b), int(e), float(lr),
                                float(d), float(l1), float(m))
                    for b, e, lr, d, l1, m in segs)


def bias_correction(beta1, beta2, step):
    """Adam's (c1, c2) = (1 / (1 - b1^t), 1 / sqrt(1 - b2^t)) of the t-th
    update: the betas as the segment table holds them (float32), the powers
    in double, the results rounded to float32."""
    b1, b2, t = _f32(beta1), _f32(beta2), int(step)
    return (_f32(1.0 / (1.0 - b1 ** t)),
            _f32(1.0 / math.sqrt(1.0 - b2 ** t)))


def _pack_solver_segs(segs, step=None):
    """SolverSeg rows (csrc/kernels/elementwise.hip) from 9-tuples (begin,
    end, lr, decay, l1, moment, mode, eps, rho).  Adam rows (modes 4, 5) also
    carry the bias correction of update number ``step``."""
    out = []
    for b, e, lr, d, l1, m, mode, eps, rho in segs:
        c1 = c2 = 0.0
        if int(mode) in _ADAM_MODES:
            if step is None or int(step) < 1:
                raise ValueError("solver_update: adam / adamw need step >= 1 "
                                 "(the 1-based update number), not %r" %
                                 (step,))
            c1, c2 = bias_correction(m, rho, step)
        out.append(struct.pack(
            "<qqffffifffffff", int(b), int(e), float(lr), float(d), float(l1),
            float(m), int(mode), float(eps), float(rho), c1, c2, 0.0, 0.0,
            0.0))
    return b"".join(out)


def _segs_tensor(raw, device):
    """Device copy of a packed segment table, from a BOUNDED cache (one-off
    callers; a training loop whose learning rates move every step uses a
    :class:`SegmentTable` instead)."""
    key = (raw, str(device))
    t = _SEG_CACHE.get(key)
    if t is None:
        t = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(device)
        if len(_SEG_CACHE) >= _SEG_CACHE_MAX:
            _SEG_CACHE.pop(next(iter(_SEG_CACHE)))
        _SEG_CACHE[key] = t
    return t


class SegmentTable(object):
    """One persistent device buffer holding a packed segment table, updated
    IN PLACE when the table changes (an LR policy such as ``exp`` changes it
    every step).  The device address never moves - a captured HIP graph of
    the train step keeps reading the current rates - and no device memory is
    allocated per step.  Host staging goes through two pinned buffers, each
    reused only after its previous stream-ordered copy has completed."""

    def __init__(self, device):
        self.device = device
        self.dev = None
        self._raw = None
        self._pinned = [None, None]
        self._events = [None, None]
        self._slot = 0

    def update(self, raw):
        if raw == self._raw and self.dev is not None:
            return self.dev
        n = len(raw)
        gpu = self.device.type == "cuda"
        if self.dev is None or self.dev.numel() < n:
            self.dev = torch.zeros(max(n, 64), dtype=torch.uint8,
                                   device=self.device)
            self._pinned = [None, None]
        if not gpu:
            self.dev[:n].copy_(torch.frombuffer(bytearray(raw),
                                                dtype=torch.uint8))
        else:
            i = self._slot
            self._slot ^= 1
            if self._events[i] is not None:
                self._events[i].synchronize()
            if self._pinned[i] is None or self._pinned[i].numel() < n:
                self._pinned[i] = torch.empty(self.dev.numel(),
                                              dtype=torch.uint8,
                                              pin_memory=True)
            self._pinned[i][:n].copy_(torch.frombuffer(bytearray(raw),
                                                       dtype=torch.uint8))
            self.dev[:n].copy_(self._pinned[i][:n], non_blocking=True)
            ev = torch.cuda.Event()
            ev.record()
            self._events[i] = ev
        self._raw = raw
        return self.dev


def _zero_from(zero_grad, n):
    """Offset from which an update clears the gradients: True -> 0 (all),
    False / None -> n (none), an int -> that offset (the split-K tail)."""
    if zero_grad is None or zero_grad is False:
        return n
    if zero_grad is True:
        return 0
    return max(0, min(int(zero_grad), n))


def sgd_update(w, grad, mom, segs, w_lp=None, gscale=1.0, zero_grad=False,
               table=None, max_blocks=None):
    """Fused multi-segment SGD (flat float32 buffers).

    segs: [(begin, end, lr, weights_decay, l1_vs_l2, gradient_moment)]
      g = grad*gscale + decay*((1-l1)*w + l1*sign(w));  v = moment*v - lr*g;
      w += v;  w_lp = bfloat16(w)
    zero_grad: True clears the whole gradient after reading it, an int
    offset clears only grad[offset:] (see :func:`_zero_from`).
    table: optional :class:`SegmentTable` the packed segments are kept in.
    max_blocks: cap on the GPU grid (a side-stream update next to compute)."""
    n = w.numel()
    zf = _zero_from(zero_grad, n)
    if _gpu(w):
        raw = _pack_sgd_segs(segs)
        st = table.update(raw) if table is not None else \
            _segs_tensor(raw, w.device)
        if mom is not None and max_blocks:
            fn = getattr(_lib.lib(), "hvk_sgd4_grid")
            if fn(_p(w), _p(grad), _p(mom), _p(w_lp), _p(st), len(segs), n,
                  float(gscale), zf, int(max_blocks), _s(w)) == 0:
                return w
        fn = getattr(_lib.lib(), "hvk_sgd4")
        if mom is not None and fn(_p(w), _p(grad), _p(mom), _p(w_lp),
                                  _p(st), len(segs), n, float(gscale),
                                  zf, _s(w)) == 0:
            return w
        _lib_call("hvk_sgd", _p(w), _p(grad), _p(mom), _p(w_lp), _p(st),
                  len(segs), n, float(gscale), _s(w))
        if zf < n:
            grad[zf:].zero_()
        return w
    for b, e, lr, d, l1, m in segs:
        ws = w[b:e]
        g = grad[b:e] * gscale
        if d:
            g = g + d * ((1 - l1) * ws + l1 * torch.sign(ws))
        v = -lr * g
        if mom is not None:
            v = v + m * mom[b:e]
            mom[b:e] = v
        ws += v
    if w_lp is not None:
        w_lp.copy_(w.to(w_lp.dtype))
    if zf < n:
        grad[zf:].zero_()
    return w


SOLVERS = {"momentum": 0, "adagrad": 1, "adadelta": 2, "rprop": 3,
           "adam": 4, "adamw": 5, "rmsprop": 6}
_ADAM_MODES = (4, 5)

_SQNORM_WS = {}
_SQNORM_WS_LEN = 2048      # one partial sum per workgroup of the first launch
_SQNORM_CHUNK = 4096       # CPU path: float32 sums of chunks, then of those


def grad_sqnorm(grad, out=None, ws=None):
    """Sum of squares of a flat float32 buffer into ``out`` (1-element
    float32 tensor on grad's device, allocated if None).  GPU: two launches,
    no atomics, bit-identical from run to run (``sqnorm_partial_kernel`` /
    ``sqnorm_finish_kernel``); ``ws``: float32 workspace of up to 2048
    elements (a per-device one is kept otherwise).  CPU: a float32 sum."""
    n = grad.numel()
    if n < 1 or grad.dtype != torch.float32 or not grad.is_contiguous():
        raise ValueError("grad_sqnorm needs a contiguous float32 buffer of "
                         "n >= 1 elements")
    if out is None:
        out = torch.empty(1, dtype=torch.float32, device=grad.device)
    if _gpu(grad):
        if ws is None:
            ws = _SQNORM_WS.get(grad.device)
            if ws is None:
                ws = _SQNORM_WS[grad.device] = torch.empty(
                    _SQNORM_WS_LEN, dtype=torch.float32, device=grad.device)
        _lib_call("hvk_grad_sqnorm", _p(grad), n, _p(ws), ws.numel(),
                  _p(out), _s(grad))
        return out
    sq = grad.reshape(-1) * grad.reshape(-1)
    k = n // _SQNORM_CHUNK * _SQNORM_CHUNK
    parts = sq[:k].view(-1, _SQNORM_CHUNK).sum(1)
    out[0] = torch.cat([parts, sq[k:].sum().reshape(1)]).sum()
    return out


def clip_scale(gscale, sqnorm, clip_norm):
    """gscale' = gscale * min(1, clip / (gscale * sqrt(sqnorm) + 1e-6)) in
    float32 operations, as every thread of the update kernel computes it
    (the rule of ``torch.nn.utils.clip_grad_norm_`` on the scaled gradient).
    ``sqnorm`` None or ``clip_norm`` <= 0: ``gscale`` (as float32)."""
    import numpy as np
    gs = np.float32(gscale)
    if sqnorm is None or not clip_norm > 0:
        return float(gs)
    with np.errstate(all="ignore"):
        nrm = gs * np.sqrt(np.float32(float(sqnorm.reshape(-1)[0])))
        coef = np.fmin(np.float32(1.0),
                       np.float32(clip_norm) / (nrm + np.float32(1e-6)))
        return float(gs * coef)


def _adam_cpu(ws, g, a, c, lr, d, l1, m, mode, eps, rho, c1, c2):
    """Modes 4 - 6 on float32 CPU views, scalar by scalar as the kernel's
    ``solver_step`` (which fuses some of the product-sums)."""
    import numpy as np
    f = np.float32
    one = f(1.0)
    if d:
        r = float(one - f(l1)) * ws + float(f(l1)) * torch.sign(ws)
        if mode == 5:
            ws -= float(f(lr) * f(d)) * r
        else:
            g = g + float(f(d)) * r
    if mode == 6:
        a.mul_(float(f(rho))).add_(float(one - f(rho)) * g * g)
        ws -= float(f(lr)) * g / (a.sqrt() + float(f(eps)))
        return
    a.mul_(float(f(m))).add_(float(one - f(m)) * g)
    c.mul_(float(f(rho))).add_(float(one - f(rho)) * g * g)
    ws -= float(f(lr) * f(c1)) * a / (c.sqrt() * c2 + float(f(eps)))


def solver_update(w, grad, s1, s2, segs, w_lp=None, gscale=1.0,
                  zero_grad=False, table=None, step=None, sqnorm=None,
                  clip_norm=0.0):
    """Fused multi-segment update with a solver per segment.

    segs: [(begin, end, lr, decay, l1_vs_l2, moment, mode, eps, rho)], modes
    in :data:`SOLVERS`.  adam / adamw: moment = beta1, rho = beta2 and
    ``step`` (>= 1) is the update number of the bias correction, which
    travels in the table; rmsprop: rho = alpha.  ``sqnorm`` (1-element
    float32 tensor, see :func:`grad_sqnorm`) with ``clip_norm`` > 0 clips
    the scaled gradient by its global norm (:func:`clip_scale`).  Tables of
    modes 0 - 3 without clipping run ``solver_kernel``, everything else
    ``solver4_kernel`` or its scalar twin (csrc/kernels/elementwise.hip)."""
    n = w.numel()
    zf = _zero_from(zero_grad, n)
    clip = float(clip_norm) if sqnorm is not None and clip_norm and \
        clip_norm > 0 else 0.0
    new = clip > 0 or any(int(sg[6]) >= 4 for sg in segs)
    if any(int(sg[6]) in _ADAM_MODES for sg in segs) and \
            (step is None or int(step) < 1):
        raise ValueError("solver_update: adam / adamw need step >= 1 (the "
                         "1-based update number), not %r" % (step,))
    if _gpu(w):
        raw = _pack_solver_segs(segs, step)
        st = table.update(raw) if table is not None else \
            _segs_tensor(raw, w.device)
        if new:
            _lib_call("hvk_solver4", _p(w), _p(grad), _p(s1), _p(s2),
                      _p(w_lp), _p(st), len(segs), n, float(gscale), zf,
                      _p(sqnorm) if clip > 0 else None, clip, _s(w))
        else:
            _lib_call("hvk_solver", _p(w), _p(grad), _p(s1), _p(s2),
                      _p(w_lp), _p(st), len(segs), n, float(gscale), zf,
                      _s(w))
        return w
    if clip > 0:
        gscale = clip_scale(gscale, sqnorm, clip)
    for b, e, lr, d, l1, m, mode, eps, rho in segs:
        ws = w[b:e]
        g = grad[b:e] * gscale
        if mode >= 4:
            c1, c2 = bias_correction(m, rho, step) if mode != 6 else (0., 0.)
            _adam_cpu(ws, g, s1[b:e], s2[b:e], lr, d, l1, m, mode, eps, rho,
                      c1, c2)
            continue
        if d:
            g = g + d * ((1 - l1) * ws + l1 * torch.sign(ws))
        a = s1[b:e]
        if mode == 1:
            a += g * g
            ws -= lr * g / (a.sqrt() + eps)
        elif mode == 2:
            c = s2[b:e]
            a.mul_(rho).add_((1 - rho) * g * g)
            dd = g * (c + eps).sqrt() / (a + eps).sqrt()
            c.mul_(rho).add_((1 - rho) * dd * dd)
            ws -= lr * dd
        elif mode == 3:
            prev = s2[b:e]
            step = torch.where(a > 0, a, torch.full_like(a, lr))
            # by the signs, not the product: tiny gradients underflow it
            same = torch.sign(prev) * torch.sign(g) > 0
            flip = torch.sign(prev) * torch.sign(g) < 0
            step = torch.where(same, (step * 1.2).clamp(max=50.0), step)
            step = torch.where(flip, (step * 0.5).clamp(min=1e-6), step)
            g = torch.where(flip, torch.zeros_like(g), g)
            ws -= torch.sign(g) * step
            a.copy_(step)
            prev.copy_(g)
        else:
            a.mul_(m).sub_(lr * g)
            ws += a
    if w_lp is not None:
        w_lp.copy_(w.to(w_lp.dtype))
    if zf < n:
        grad[zf:].zero_()
    return w


# ---------------------------------------------------------------- dropout
def _hash32(i, seed):
    M = 0xFFFFFFFF
    x = i ^ ((seed * 0x9E3779B9) & M)
    x ^= x >> 16
    x = (x * 0x7feb352d) & M
    x ^= x >> 15
    x = (x * 0x846ca68b) & M
    x ^= x >> 16
    return x


def _f32(x):
    """x rounded to float32, as the kernel library receives it."""
    return struct.unpack("<f", struct.pack("<f", float(x)))[0]


def dropout_thresh(p):
    """Elements whose hash is >= this are kept: floor(float32(p) * 2^32),
    at most 2^32 - 1 (the rule of the hvk_dropout* entries)."""
    return max(0, min(0xFFFFFFFF, int(_f32(p) * 4294967296.0)))


def dropout_mask_ref(n, seed, p, base=0):
    i = (torch.arange(n, dtype=torch.int64) + int(base)) & 0xFFFFFFFF
    h = _hash32(i, int(seed) & 0xFFFFFFFF)
    return h >= dropout_thresh(p)


def dropout(x, p, seed, out=None, seed_dev=None, base=0):
    """y = x * keep / (1-p) with a counter-based mask (same seed -> same mask:
    the backward pass calls this on dy).  ``seed_dev``: a 1-element int32
    device tensor holding the seed instead (graph-safe, see
    :func:`seed_advance`); ``seed`` is then ignored.  ``base``: mask index
    of element 0 (a data-parallel rank's offset in the global minibatch)."""
    if out is None:
        out = torch.empty_like(x)
    if seed_dev is not None and not _gpu(x):
        seed = int(seed_dev.reshape(-1)[0]) & 0xFFFFFFFF
    if _gpu(x):
        if seed_dev is not None:
            if base:
                _lib_call("hvk_dropout_dev_at", _p(x), DT[x.dtype], _p(out),
                          DT[out.dtype], x.numel(), _p(seed_dev), float(p),
                          int(base), _s(x))
                return out
            _lib_call("hvk_dropout_dev", _p(x), DT[x.dtype], _p(out),
                      DT[out.dtype], x.numel(), _p(seed_dev), float(p), None,
                      _s(x))
            return out
        if base:
            raise ValueError("dropout: base needs the device seed path")
        _lib_call("hvk_dropout", _p(x), DT[x.dtype], _p(out), DT[out.dtype],
                  x.numel(), int(seed) & 0xFFFFFFFF, float(p), None, _s(x))
        return out
    keep = dropout_mask_ref(x.numel(), seed, p, base).view(x.shape)
    # the float32 scale of the kernel entries; dropped elements are +0
    one, p32 = torch.ones((), dtype=torch.float32), torch.tensor(
        _f32(p), dtype=torch.float32)
    scale = one / (one - p32) if p32 < 1 else torch.zeros(())
    xf = x.float()
    out.copy_(torch.where(keep, xf * scale, torch.zeros_like(xf))
              .to(out.dtype))
    return out


def seed_advance_ref(seed):
    """Host mirror of hvk_seed_advance: seed <- hash32(seed + 1)."""
    i = torch.tensor([(int(seed) + 1) & 0xFFFFFFFF], dtype=torch.int64)
    return int(_hash32(i, 0x2545F491)[0])


def seed_advance(seed_dev):
    """Advance a device-resident dropout seed (int32 [1]) in place - a
    stream-ordered kernel, so a captured step draws a new mask every
    replay."""
    if _gpu(seed_dev):
        _lib_call("hvk_seed_advance", _p(seed_dev), _s(seed_dev))
        return seed_dev
    v = seed_advance_ref(int(seed_dev.reshape(-1)[0]) & 0xFFFFFFFF)
    seed_dev.fill_(v - (1 << 32) if v >= (1 << 31) else v)
    return seed_dev


def trace_marker(tag=0, stream=None):
    """Launch the empty marker kernel on ``stream`` (default: the current
    one; bench.py --mark-steps passes the workflow's compute stream) to
    bracket the timed steps in a rocprofv3 kernel trace."""
    if torch.cuda.is_available():
        st = stream if stream is not None else torch.cuda.current_stream()
        _lib_call("hvk_trace_marker", int(tag), st.cuda_stream)


# --------------------------------------------------------------------- RNG
def xorshift1024star(states, rounds, out=None):
    """states: int64 [n,16] (raw uint64 bits, updated in place); returns int64
    [rounds*16*n] laid out out[round*16*n + i*n + id]."""
    n = states.shape[0]
    if out is None:
        out = torch.empty(rounds * 16 * n, dtype=torch.int64,
                          device=states.device)
    if _gpu(states):
        _lib_call("hvk_xorshift1024star", _p(states), n, int(rounds), _p(out),
                  _s(states))
        return out
    from veles_amd.prng.random_generator import xorshift1024star as ref
    s = states.numpy().view("uint64")
    r = ref(s, rounds)
    out.copy_(torch.from_numpy(r.view("int64")))
    return out


def xorshift128plus(states, out=None):
    n = states.shape[0]
    if out is None:
        out = torch.empty(n, dtype=torch.int64, device=states.device)
    if _gpu(states):
        _lib_call("hvk_xorshift128plus", _p(states), n, _p(out), _s(states))
        return out
    from veles_amd.prng.random_generator import xorshift128plus as ref
    r = ref(states.numpy().view("uint64"), 1)
    out.copy_(torch.from_numpy(r.view("int64")))
    return out


# ------------------------------------------------------------- data moving
def join(inputs, out=None):
    """Feature-wise concatenation of [B, n_i] inputs (InputJoiner)."""
    B = inputs[0].shape[0]
    lens = [t.numel() // B for t in inputs]
    if out is None:
        out = torch.empty(B, sum(lens), dtype=inputs[0].dtype,
                          device=inputs[0].device)
    if _gpu(out) and len(inputs) <= 16:
        import ctypes
        arr = (ctypes.c_void_p * len(inputs))(*[t.data_ptr() for t in inputs])
        la = (ctypes.c_int * len(inputs))(*lens)
        _lib_call("hvk_join", ctypes.cast(arr, ctypes.c_void_p),
                  ctypes.cast(la, ctypes.c_void_p), len(inputs),
                  DT[out.dtype], _p(out), B, _s(out))
        return out
    out.copy_(torch.cat([t.reshape(B, -1).to(out.dtype) for t in inputs], 1))
    return out


def cast(x, dtype, scale=1.0, out=None):
    if out is None:
        out = torch.empty(x.shape, dtype=dtype, device=x.device)
    if _gpu(x) and x.dtype in DT and out.dtype in DT:
        _lib_call("hvk_cast", _p(x), DT[x.dtype], _p(out), DT[out.dtype],
                  x.numel(), float(scale), _s(x))
        return out
    out.copy_((x.float() * scale).to(dtype))
    return out


def fill_minibatch(src, shuffled, start, count, dst, *, mean=None,
                   rdisp=None, labels=None, labels_out=None, idx_out=None):
    """Gather a minibatch: dst[i] = (src[shuffled[start+i]] - mean) * rdisp
    for i < count, zeros after; labels/indices gathered (-1 padding)."""
    max_mb = dst.shape[0]
    sample = src.numel() // src.shape[0]
    if _gpu(dst):
        _lib_call("hvk_fill_minibatch", _p(src), DT[src.dtype], _p(shuffled),
                  int(start), int(count), max_mb, sample, _p(mean), _p(rdisp),
                  _p(dst), DT[dst.dtype], _p(labels), _p(labels_out),
                  _p(idx_out), _s(dst))
        return dst
    idx = shuffled[start:start + count].long()
    v = src.reshape(src.shape[0], -1)[idx].float()
    if mean is not None:
        v = v - mean.reshape(1, -1).float()
    if rdisp is not None:
        v = v * rdisp.reshape(1, -1).float()
    d = dst.view(max_mb, -1)
    d[:count] = v.to(dst.dtype)
    d[count:] = 0
    if labels_out is not None:
        labels_out[:count] = labels[idx] if labels is not None else -1
        labels_out[count:] = -1
    if idx_out is not None:
        idx_out[:count] = idx.to(idx_out.dtype)
        idx_out[count:] = -1
    return dst


def image_batch_ref(src, idx, params, Ho, Wo, sobel=False, mean=None,
                    rdisp=None, bg=None, bgcolor=None):
    """Torch (f32) reference of hvk_image_batch: crop (cy, cx) -> mirror ->
    rotate (bilinear, cv2 centre and angle convention) -> optional Sobel
    magnitude channel -> (v - mean) * rdisp.  src uint8 [N][Hs][Ws][C];
    params [B][6] = (cy, cx, cos, sin, mirror, -)."""
    N, Hs, Ws, C = src.shape
    B = idx.shape[0]
    dev = src.device
    p = params.float()
    oy = torch.arange(Ho, device=dev, dtype=torch.float32).view(1, Ho, 1)
    ox = torch.arange(Wo, device=dev, dtype=torch.float32).view(1, 1, Wo)

    def sample(yy, xx):
        cy, cx = p[:, 0].view(B, 1, 1), p[:, 1].view(B, 1, 1)
        ct, st = p[:, 2].view(B, 1, 1), p[:, 3].view(B, 1, 1)
        mir = (p[:, 4] != 0).view(B, 1, 1)
        ccx, ccy = float(Wo // 2), float(Ho // 2)
        dx, dy = xx - ccx, yy - ccy
        sx = ccx + ct * dx - st * dy
        sy = ccy + st * dx + ct * dy
        sx = torch.where(mir, (Wo - 1) - sx, sx)
        x0, y0 = torch.floor(sx), torch.floor(sy)
        axx, ayy = sx - x0, sy - y0
        v = torch.zeros(B, Ho, Wo, C, device=dev)
        can = src[idx.clamp_min(0).long()].float()   # [B,Hs,Ws,C]
        for t in range(4):
            ty, tx = t >> 1, t & 1
            w = (ayy if ty else 1 - ayy) * (axx if tx else 1 - axx)
            yi, xi = (y0 + ty).long(), (x0 + tx).long()
            inb = (yi >= 0) & (yi < Ho) & (xi >= 0) & (xi < Wo) & \
                (cy.long() + yi < Hs) & (cx.long() + xi < Ws)
            gy = (cy.long() + yi).clamp(0, Hs - 1)
            gx = (cx.long() + xi).clamp(0, Ws - 1)
            bi = torch.arange(B, device=dev).view(B, 1, 1).expand_as(gy)
            val = can[bi, gy, gx]                      # [B,Ho,Wo,C]
            if bg is not None:
                bgv = bg.float()[yi.clamp(0, Ho - 1), xi.clamp(0, Wo - 1)]
            elif bgcolor is not None:
                bgv = bgcolor.float().view(1, 1, 1, C).expand_as(val)
            else:
                bgv = torch.zeros_like(val)
            val = torch.where(inb.unsqueeze(-1), val, bgv)
            v = v + w.unsqueeze(-1) * val
        return v

    yy = oy.expand(B, Ho, Wo)
    xx = ox.expand(B, Ho, Wo)
    v = sample(yy, xx)
    if sobel:
        def gray(a):
            return (0.299 * a[..., 0] + 0.587 * a[..., 1] + 0.114 * a[..., 2]
                    if C >= 3 else a[..., 0])
        g = {}
        for t in range(9):
            ry = (yy + (t // 3 - 1)).clamp(0, Ho - 1)
            rx = (xx + (t % 3 - 1)).clamp(0, Wo - 1)
            g[t] = gray(sample(ry, rx))
        gx = (g[2] + 2 * g[5] + g[8]) - (g[0] + 2 * g[3] + g[6])
        gy = (g[6] + 2 * g[7] + g[8]) - (g[0] + 2 * g[1] + g[2])
        v = torch.cat([v, torch.sqrt(gx * gx + gy * gy).unsqueeze(-1)], -1)
    if mean is not None:
        v = v - mean.float().view(1, Ho, Wo, -1)
    if rdisp is not None:
        v = v * rdisp.float().view(1, Ho, Wo, -1)
    return v * (idx >= 0).float().view(B, 1, 1, 1)


def image_batch(src, idx, params, out, sobel=False, mean=None, rdisp=None,
                bg=None, bgcolor=None):
    """Augmented, normalised image minibatch from uint8 canvases (the image
    loaders' device path, hvk_image_batch): out [B][Ho][Wo][C + sobel]."""
    B, Ho, Wo = out.shape[0], out.shape[1], out.shape[2]
    N, Hs, Ws, C = src.shape
    if _gpu(out):
        _lib_call("hvk_image_batch", _p(src), Hs * Ws * C, Hs, Ws, C,
                  _p(idx), _p(params), B, Ho, Wo, 1 if sobel else 0,
                  _p(mean), _p(rdisp), _p(bg), _p(bgcolor), _p(out), _s(out))
        return out
    out.copy_(image_batch_ref(src, idx, params, Ho, Wo, sobel, mean, rdisp,
                              bg, bgcolor).to(out.dtype))
    return out


def mean_disp_normalize(x, mean, rdisp, out=None, out_dtype=None):
    """out = (float(x) - mean) * rdisp, mean/rdisp broadcast per sample."""
    if out is None:
        out = torch.empty(x.shape, dtype=out_dtype or torch.float32,
                          device=x.device)
    sample = mean.numel()
    if _gpu(x):
        _lib_call("hvk_mean_disp_normalize", _p(x), DT[x.dtype], _p(mean),
                  _p(rdisp), _p(out), DT[out.dtype], x.numel(), sample, _s(x))
        return out
    v = (x.float().reshape(-1, sample) - mean.reshape(1, -1).float()) * \
        rdisp.reshape(1, -1).float()
    out.copy_(v.reshape(out.shape).to(out.dtype))
    return out


# ------------------------------------------------------------- Kohonen maps
# docs/OPS.md "Kohonen maps"; kernels in csrc/kernels/kohonen.hip.
_KOH_TILE = 128          # neurons per tile of both kernels
_KOH_XTILE = 64          # samples (winner search) / features (update) per tile
_KOH_KTILE = 32          # batch rows per K tile of the update
_KOH_WGS = 512           # workgroups wanted before a kernel stops splitting
_KOH_WS_MAX = 1 << 26    # floats: cap of the update's slice workspace


def kohonen_coords(sx, sy, device="cpu"):
    """Grid positions float32 [sx * sy][2] of a rectangular map: neuron
    n = y * sx + x sits at ((x - (sx-1)/2) h, (y - (sy-1)/2) h) with
    h = 2 / max(sx-1, sy-1, 1), so the long side spans [-1, 1]."""
    sx, sy = int(sx), int(sy)
    if sx < 1 or sy < 1:
        raise ValueError("kohonen_coords: shape (%d, %d)" % (sx, sy))
    h = 2.0 / max(sx - 1, sy - 1, 1)
    gx = (torch.arange(sx, dtype=torch.float64) - (sx - 1) / 2.0) * h
    gy = (torch.arange(sy, dtype=torch.float64) - (sy - 1) / 2.0) * h
    c = torch.stack([gx.repeat(sy), gy.repeat_interleave(sx)], 1)
    return c.to(torch.float32).to(device)


def _kohonen_args(name, x, w, n):
    """Shared host checks; returns (x as [rows][D], rows used, NN, D)."""
    if w.dtype != torch.float32 or w.dim() != 2:
        raise ValueError("%s: weights must be float32 [NN][D], got %s %s" %
                         (name, w.dtype, tuple(w.shape)))
    if x.dtype not in (torch.float32, torch.bfloat16):
        raise ValueError("%s: input must be float32 or bfloat16, got %s" %
                         (name, x.dtype))
    if x.dim() < 1 or x.shape[0] < 1:
        raise ValueError("%s: empty input %s" % (name, tuple(x.shape)))
    if not x.is_contiguous() or not w.is_contiguous():
        raise ValueError("%s: input and weights must be contiguous" % name)
    if x.device != w.device:
        raise ValueError("%s: input on %s, weights on %s" %
                         (name, x.device, w.device))
    NN, D = w.shape
    x2 = x.view(x.shape[0], -1)
    if NN < 1 or D < 1 or x2.shape[1] != D:
        raise ValueError("%s: input %s does not match weights %s" %
                         (name, tuple(x.shape), tuple(w.shape)))
    n = x2.shape[0] if n is None else int(n)
    if n < 1 or n > x2.shape[0]:
        raise ValueError("%s: %d valid rows of %d" % (name, n, x2.shape[0]))
    if n * D >= 1 << 31 or NN * D >= 1 << 31:
        raise ValueError("%s: %d x %d input / %d x %d weights exceed 2^31 "
                         "elements" % (name, n, D, NN, D))
    return x2, n, NN, D


def _kohonen_out(name, what, t, dtype, size, device):
    if t is None:
        return None
    if t.dtype != dtype or t.dim() != 1 or t.shape[0] < size or \
            not t.is_contiguous() or t.device != device:
        raise ValueError("%s: %s must be a contiguous %s [>= %d] on %s" %
                         (name, what, dtype, size, device))
    return t


def _kohonen_fn(name):
    fn = getattr(_lib.lib(), name, None)
    if fn is None:
        raise _lib.KernelLibraryMissing(
            "%s lacks %s - rebuild with python -m veles_amd.ops.build" %
            (_lib.LIB_PATH, name))
    return fn


def kohonen_argmin(x, w, n=None, argmin=None, qerr=None, winners=None,
                   splits=0):
    """Winners of the first ``n`` rows of ``x`` on the map ``w`` (float32
    [NN][D]): argmin[b] = argmin_n (|w[n]|^2 - 2 x[b].w[n]), ties to the
    lowest n.  ``qerr`` (float32) receives max(0, |x[b]|^2 + that minimum),
    ``winners`` (int32 [NN]) is incremented at every winner.  ``splits``
    forces the number of neuron slices on the GPU (0: chosen).  Returns the
    int32 winners, a view of ``argmin`` when that is given."""
    name = "kohonen_argmin"
    x2, n, NN, D = _kohonen_args(name, x, w, n)
    dev = w.device
    if argmin is None:
        argmin = torch.empty(n, dtype=torch.int32, device=dev)
    _kohonen_out(name, "argmin", argmin, torch.int32, n, dev)
    _kohonen_out(name, "qerr", qerr, torch.float32, n, dev)
    _kohonen_out(name, "winners", winners, torch.int32, NN, dev)
    splits = int(splits)
    if splits < 0:
        raise ValueError("%s: splits %d" % (name, splits))
    if _gpu(w):
        tb = -(-n // _KOH_XTILE)
        nt = -(-NN // _KOH_TILE)
        sp = max(1, min(splits or _KOH_WGS // tb, nt))
        ws = _grow_ws("kohonen_argmin", (2 * sp + 1) * n, torch.float32, dev)
        _lib.check(_kohonen_fn("hvk_kohonen_argmin")(
            _p(x2), DT[x2.dtype], _p(w), n, NN, D, D, _p(argmin), _p(qerr),
            _p(winners), _p(ws), sp, _s(w)), "hvk_kohonen_argmin")
        return argmin[:n]
    xs = x2[:n].float()
    s = (w * w).sum(1).unsqueeze(0) - 2.0 * (xs @ w.t())
    a = s.argmin(1)      # the first of equal minima
    argmin[:n] = a.to(torch.int32)
    if qerr is not None:
        v = s.gather(1, a.unsqueeze(1)).squeeze(1)
        qerr[:n] = ((xs * xs).sum(1) + v).clamp_(min=0)
    if winners is not None:
        winners[:NN] += torch.bincount(a, minlength=NN).to(torch.int32)
    return argmin[:n]


def kohonen_update(x, w, coords, argmin, sigma, gradient, n=None, splits=0):
    """One neighbourhood step on ``w`` in place, over the first ``n`` rows:
    w[m] += (gradient / n) * sum_b G[b][m] (x[b] - w[m]) with G[b][m] =
    exp(-|coords[m] - coords[argmin[b]]|^2 / (2 sigma^2)).  Indices outside
    the map are clamped into it.  ``splits`` forces the number of batch
    slices on the GPU (0: chosen)."""
    name = "kohonen_update"
    x2, n, NN, D = _kohonen_args(name, x, w, n)
    dev = w.device
    if coords.dtype != torch.float32 or tuple(coords.shape) != (NN, 2) or \
            not coords.is_contiguous() or coords.device != dev:
        raise ValueError("%s: coords must be a contiguous float32 [%d][2] on "
                         "%s" % (name, NN, dev))
    _kohonen_out(name, "argmin", argmin, torch.int32, n, dev)
    sigma, gradient, splits = float(sigma), float(gradient), int(splits)
    if not sigma > 0 or splits < 0:
        raise ValueError("%s: sigma %r, splits %d" % (name, sigma, splits))
    inv2s2 = 1.0 / (2.0 * sigma * sigma)
    if _gpu(w):
        tiles = -(-NN // _KOH_TILE) * -(-D // _KOH_XTILE)
        nk = -(-n // _KOH_KTILE)
        sp = splits
        if not sp:
            sp = min(_KOH_WGS // tiles, nk // 4)
            while sp > 1 and sp * NN * (D + 1) > _KOH_WS_MAX:
                sp //= 2
        sp = max(1, min(sp, nk))
        ws = None if sp == 1 else _grow_ws(
            "kohonen_update", sp * NN * (D + 1), torch.float32, dev)
        _lib.check(_kohonen_fn("hvk_kohonen_update")(
            _p(x2), DT[x2.dtype], _p(w), _p(coords), _p(argmin), n, NN, D, D,
            inv2s2, gradient / n, _p(ws), sp, _s(w)), "hvk_kohonen_update")
        return w
    xs = x2[:n].float()
    a = argmin[:n].long().clamp_(0, NN - 1)
    d = coords.unsqueeze(1) - coords.unsqueeze(0)
    K = torch.exp(-(d * d).sum(2) * inv2s2)
    G = K[a]                                   # [n][NN]
    w += (gradient / n) * (G.t() @ xs - G.sum(0).unsqueeze(1) * w)
    return w


# --------------------------------------------------------- recurrent layers
# docs/OPS.md "Recurrent layers"; kernels in csrc/kernels/recurrent.hip.
_CELLS = {"lstm": (0, 4), "rnn": (1, 1)}   # cell -> (kernel code, gates)


def _r8(n):
    return -(-n // 8) * 8


def _rec_fn(name):
    fn = getattr(_lib.lib(), name, None)
    if fn is None:
        raise _lib.KernelLibraryMissing(
            "%s lacks %s - rebuild with python -m veles_amd.ops.build" %
            (_lib.LIB_PATH, name))
    return fn


def _rec_buf(store, key, shape, dtype, dev, zero=False):
    """store[key] when it fits, else a new tensor put there: a caller that
    keeps ``store`` gets the same buffers at every call"""
    t = store.get(key)
    if t is None or tuple(t.shape) != tuple(shape) or t.dtype != dtype or \
            t.device != dev:
        t = (torch.zeros if zero else torch.empty)(shape, dtype=dtype,
                                                   device=dev)
        store[key] = t
    return t


def _lstm_args(name, x, w, bias, H, cell, D):
    """Shared host checks of lstm_fwd / lstm_bwd over ``D`` directions;
    returns (B, T, I, H, kernel cell code, gates)."""
    if cell not in _CELLS:
        raise ValueError("%s: unknown cell %r (lstm, rnn)" % (name, cell))
    code, ng = _CELLS[cell]
    H = int(H)
    if x.dim() != 3 or min(x.shape) < 1:
        raise ValueError("%s: input must be [B][T][I], got %s" %
                         (name, tuple(x.shape)))
    B, T, I = x.shape
    if H < 1 or w.dim() != 2 or tuple(w.shape) != (D * ng * H, I + H):
        raise ValueError("%s: weights must be [%d][%d] (%s, I = %d, H = %d), "
                         "got %s" % (name, D * ng * H, I + H, cell, I, H,
                                     tuple(w.shape)))
    if x.device != w.device or (bias is not None and bias.device != w.device):
        raise ValueError("%s: operands on different devices" % name)
    if x.stride(2) != 1 or x.stride(0) != T * x.stride(1) or w.stride(1) != 1:
        raise ValueError("%s: input rows must be contiguous with one pitch "
                         "over [B][T], weight rows contiguous (strides %s, "
                         "%s)" % (name, x.stride(), w.stride()))
    if bias is not None and (tuple(bias.shape) != (D * ng * H,) or
                             not bias.is_contiguous()):
        raise ValueError("%s: bias must be a contiguous [%d], got %s" %
                         (name, D * ng * H, tuple(bias.shape)))
    if _gpu(w):
        if x.dtype != torch.bfloat16 or w.dtype != torch.bfloat16:
            raise TypeError("%s: GPU input and weights must be bfloat16, got "
                            "%s / %s" % (name, x.dtype, w.dtype))
        if bias is not None and bias.dtype != torch.float32:
            raise TypeError("%s: GPU bias must be float32, got %s" %
                            (name, bias.dtype))
        if x.data_ptr() % 2 or w.data_ptr() % 2:
            raise ValueError("%s: operands off the element grid" % name)
    elif not (x.is_floating_point() and w.is_floating_point()):
        raise TypeError("%s: floating-point operands, got %s / %s" %
                        (name, x.dtype, w.dtype))
    if B * T * max(_r8(D * ng * H), x.stride(1)) >= 1 << 31:
        raise ValueError("%s: %d x %d x %d exceeds 2^31 elements" %
                         (name, B, T, max(D * ng * H, I)))
    return B, T, I, H, code, ng


def _rows(x, B, T):
    """[B][T][I] with one row pitch as a [B*T][I] view (no copy)"""
    return x.as_strided((B * T, x.shape[2]), (x.stride(1), 1))


def _gru_args(name, x, w, bias, H, D):
    """Shared host checks of gru_fwd / gru_bwd over ``D`` directions; returns
    (B, T, I, H)."""
    H = int(H)
    if x.dim() != 3 or min(x.shape) < 1:
        raise ValueError("%s: input must be [B][T][I], got %s" %
                         (name, tuple(x.shape)))
    B, T, I = x.shape
    if H < 1 or w.dim() != 2 or tuple(w.shape) != (D * 3 * H, I + H):
        raise ValueError("%s: weights must be [%d][%d] (I = %d, H = %d), "
                         "got %s" % (name, D * 3 * H, I + H, I, H,
                                     tuple(w.shape)))
    if x.device != w.device or (bias is not None and bias.device != w.device):
        raise ValueError("%s: operands on different devices" % name)
    if x.stride(2) != 1 or x.stride(0) != T * x.stride(1) or w.stride(1) != 1:
        raise ValueError("%s: input rows must be contiguous with one pitch "
                         "over [B][T], weight rows contiguous (strides %s, "
                         "%s)" % (name, x.stride(), w.stride()))
    if bias is not None and (tuple(bias.shape) != (D * 4 * H,) or
                             not bias.is_contiguous()):
        raise ValueError("%s: bias must be a contiguous [%d] = (b_r, b_z, "
                         "b_n, b_hn) per direction, got %s" %
                         (name, D * 4 * H, tuple(bias.shape)))
    if _gpu(w):
        if x.dtype != torch.bfloat16 or w.dtype != torch.bfloat16:
            raise TypeError("%s: GPU input and weights must be bfloat16, got "
                            "%s / %s" % (name, x.dtype, w.dtype))
        if bias is not None and bias.dtype != torch.float32:
            raise TypeError("%s: GPU bias must be float32, got %s" %
                            (name, bias.dtype))
        if x.data_ptr() % 2 or w.data_ptr() % 2:
            raise ValueError("%s: operands off the element grid" % name)
    elif not (x.is_floating_point() and w.is_floating_point()):
        raise TypeError("%s: floating-point operands, got %s / %s" %
                        (name, x.dtype, w.dtype))
    if B * T * max(_r8(D * 3 * H), x.stride(1)) >= 1 << 31:
        raise ValueError("%s: %d x %d x %d exceeds 2^31 elements" %
                         (name, B, T, max(D * 3 * H, I)))
    return B, T, I, H


# Directions (docs/OPS.md "Bidirectional"): every pass below is written once,
# over a list of D = 1 or 2 directions.  A direction is (d, rev): its block
# index along every direction-major axis and whether its chain runs
# t = T-1 .. 0.  Every wide buffer is [B][T][D*W] with direction d at
# [..., d*W:(d+1)*W] (W = H or NG*H; the pitch of the private padded ones is
# D*W rounded up to 8), so the kernels write both halves of a [B][T][2H]
# output through their row pitches: no flip, no concat.
_DIRS = {"forward": ((0, False),), "reverse": ((0, True),),
         "both": ((0, False), (1, True))}

# "both": one paired launch per step (True) or the chain of 2T one-direction
# launches over the same buffers (False; the A/B of tools/bench_birecurrent)
_BI_PAIRED = True


def set_birecurrent_paired(on):
    """``direction="both"`` through the paired step launches (default) or
    through one-direction launches, two per step; returns the old value."""
    global _BI_PAIRED
    old, _BI_PAIRED = _BI_PAIRED, bool(on)
    return old


def _directions(name, direction):
    if direction not in _DIRS:
        raise ValueError("%s: unknown direction %r (forward, reverse, both)" %
                         (name, direction))
    return _DIRS[direction]


def _rec_steps(fn1, fn2, name, head, dirs, T, step, stream):
    """The T step launches of one pass: ``step(d, rev, s)`` is the operand
    list of direction (d, rev) at launch ``s`` of its chain; whatever does
    not depend on ``s`` is the caller's to hoist out of ``step``."""
    if len(dirs) == 2 and _BI_PAIRED:
        for s in range(T):
            rc = fn2(*head, *step(0, False, s), *step(1, True, s), stream)
            if rc:
                _lib.check(rc, name + "2")
        return
    for s in range(T):
        for d, rev in dirs:
            rc = fn1(*head, *step(d, rev, s), stream)
            if rc:
                _lib.check(rc, name)


def _rec_last(h_all, dirs, H, T, out):
    """The final state of every direction, [h^f_{T-1} | h^r_0] for "both",
    into ``out`` or a new contiguous tensor"""
    if out is None:
        out = torch.empty(h_all.shape[0], len(dirs) * H, dtype=h_all.dtype,
                          device=h_all.device)
    for d, rev in dirs:
        out[:, d * H:(d + 1) * H].copy_(
            h_all[:, 0 if rev else T - 1, d * H:(d + 1) * H])
    return out


def _rec_hprev(save, h_all, dirs, B, T, H):
    """The chain's previous h of every row: h shifted by one step towards the
    chain's end, zeros at its first step (the buffer is zeroed once and those
    rows are never written)."""
    hp = _rec_buf(save, "_hprev", tuple(h_all.shape), h_all.dtype,
                  h_all.device, zero=True)
    if T > 1:
        for d, rev in dirs:
            sl = slice(d * H, (d + 1) * H)
            if rev:
                hp[:, :T - 1, sl].copy_(h_all[:, 1:, sl])
            else:
                hp[:, 1:, sl].copy_(h_all[:, :T - 1, sl])
    return hp


# Host checks that the forward passes and the backward passes of both cell
# families share; W = D*NG*H, DH = D*H, NB = the length of the bias gradient.
def _rec_out_check(name, out, B, DH, dev):
    if out is not None and (tuple(out.shape) != (B, DH) or out.device != dev):
        raise ValueError("%s: out must be [%d][%d] on %s" % (name, B, DH, dev))


def _rec_grad_check(name, accumulate, err, dw, dbias, B, T, DH, W, K, NB, dev):
    """``accumulate``, ``err``, ``dw`` [W][K] and ``dbias`` [NB] of a backward
    pass; returns whether ``err`` holds every step"""
    if accumulate not in (True, "overwrite"):
        raise ValueError("%s: accumulate must be True or \"overwrite\"" %
                         name)
    seq = err.dim() == 3
    if tuple(err.shape) != ((B, T, DH) if seq else (B, DH)) or \
            err.stride(-1) != 1 or err.device != dev:
        raise ValueError("%s: err must be [%d][%d] or [%d][%d][%d] with "
                         "contiguous rows on %s, got %s" %
                         (name, B, DH, B, T, DH, dev, tuple(err.shape)))
    if dw.dtype != torch.float32 or tuple(dw.shape) != (W, K) or \
            dw.stride(1) != 1 or dw.device != dev:
        raise ValueError("%s: dw must be float32 [%d][%d] on %s" %
                         (name, W, K, dev))
    if dbias is not None and (dbias.dtype != torch.float32 or
                              tuple(dbias.shape) != (NB,) or
                              not dbias.is_contiguous() or
                              dbias.device != dev):
        raise ValueError("%s: dbias must be a contiguous float32 [%d] on %s"
                         % (name, NB, dev))
    return seq


def _rec_save_check(name, fwd, save, need, dev):
    """every (key, shape, dtype) of ``need`` is in ``save`` as ``fwd`` left it"""
    for k, shape, dt in need:
        t = None if save is None else save.get(k)
        if t is None or tuple(t.shape) != shape or t.dtype != dt or \
                t.device != dev:
            raise ValueError("%s: save[%r] must be %s %s from %s" %
                             (name, k, dt, shape, fwd))


def _rec_err_input_check(name, err_input, B, T, I, hdt, dev):
    if err_input is not None and (
            tuple(err_input.shape) != (B, T, I) or
            not err_input.is_contiguous() or err_input.device != dev or
            err_input.dtype != hdt):
        raise ValueError("%s: err_input must be a contiguous %s [%d][%d][%d]"
                         % (name, hdt, B, T, I))


def _rec_err_input(err_input, dg2, w, B, T, I, hdt, dev):
    """err_input [B][T][I] = dG.Wx, summed over the directions inside the one
    product; into the caller's tensor or a new one"""
    if err_input is None:
        err_input = torch.empty(B, T, I, dtype=hdt, device=dev)
    gemm(dg2, w[:, :I], out=err_input.view(B * T, I))
    return err_input


def _rec_gates_check(name, fwd, save, shape):
    """save["_gates"] is the padded buffer that save["gates"] is a view of"""
    g_ = save.get("_gates")
    if g_ is None or tuple(g_.shape) != shape or \
            g_.data_ptr() != save["gates"].data_ptr():
        raise ValueError("%s: save[\"gates\"] is not %s's" % (name, fwd))
    return g_


def lstm_fwd(x, w, bias, H, *, cell="lstm", return_sequences=False,
             save=None, out=None, ws=None, direction="forward"):
    """Forward of a recurrent layer over ``x`` [B][T][I] (batch-major).

    ``direction`` is "forward" (D = 1 direction, the chain t = 0 .. T-1),
    "reverse" (D = 1: the same cell from t = T-1 down to 0,
    h^r_t = cell(x_t, h^r_{t+1}), output aligned with the input's time axis)
    or "both" (D = 2).  ``w`` [D*NG*H][I+H] and ``bias`` [D*NG*H] (or None)
    are direction-major; each block is ONE parameter of the one-direction
    layout: ``w[:, :I]`` is Wx, ``w[:, I:]`` is Wh; NG = 4 gates in the order
    i, f, g, o for ``cell="lstm"``, 1 for ``"rnn"``.  h and c start at zero.

        lstm: (i, f, o) = sigmoid, g = tanh of x_t.Wx^T + bias + h_{t-1}.Wh^T
              c_t = f c_{t-1} + i g,  h_t = o tanh(c_t)
        rnn:  h_t = tanh(x_t.Wx^T + bias + h_{t-1}.Wh^T)

    One GEMM projects all B*T rows of every direction (float32 ``xg``), then
    T step launches run on the current stream with no host synchronisation
    (capturable); "both" advances the two chains in one paired launch per
    step (forward chain at t = s, reverse chain at t = T-1-s).  Returns every
    h_t [B][T][D*H] = [h^f_t | h^r_t] with ``return_sequences``, else the
    final state of every direction [B][D*H] = [h^f_{T-1} | h^r_0] (``out``
    when given).  ``save`` (a dict) receives "h" [B][T][D*H], "c" [B][T][D*H]
    float32, "gates" [B][T][D*NG*H] (post-activation; lstm only) and "xg" for
    lstm_bwd, direction d of an axis of width D*W at ``[..., d*W:(d+1)*W]``;
    with ``save=None`` the gates are not written.  A kept ``save`` / ``ws``
    dict is reused: no allocation from the second call on."""
    name = "lstm_fwd"
    dirs = _directions(name, direction)
    D = len(dirs)
    B, T, I, H, code, ng = _lstm_args(name, x, w, bias, H, cell, D)
    dev = x.device
    st = save if save is not None else (ws if ws is not None else {})
    gh = ng * H
    W, DH = D * gh, D * H
    lstm = ng == 4
    if not return_sequences:
        _rec_out_check(name, out, B, DH, dev)
    if _gpu(x):
        fn1 = _rec_fn("hvk_lstm_step_fwd")
        fn2 = _rec_fn("hvk_lstm_step_fwd2") if D == 2 else None
        PW = _r8(W)
        xg_ = _rec_buf(st, "_xg", (B, T, PW), torch.float32, dev)
        h_all = _rec_buf(st, "h", (B, T, DH), torch.bfloat16, dev)
        c_all = _rec_buf(st, "c", (B, T, DH), torch.float32, dev) \
            if lstm else None
        g_ = _rec_buf(st, "_gates", (B, T, PW), torch.bfloat16, dev) \
            if lstm and save is not None else None
        gemm(_rows(x, B, T), w[:, :I], trans_b=True, bias=bias,
             out=xg_.view(B * T, PW)[:, :W])
        ph, pc, pxg = h_all.data_ptr(), _p(c_all), xg_.data_ptr()
        pg = _p(g_)
        ldw, ldh, ldp = w.stride(0), T * DH, T * PW
        pw = [w.data_ptr() + 2 * (I + d * gh * ldw) for d in range(D)]

        def step(d, rev, s):
            t = T - 1 - s if rev else s
            a, ag = t * DH + d * H, t * PW + d * gh     # row t of direction d
            ap = a + DH if rev else a - DH              # the chain's previous
            return (ph + 2 * ap if s else None, ldh, pw[d], ldw,
                    pxg + 4 * ag, ldp,
                    pc + 4 * ap if lstm and s else None, ldh,
                    pc + 4 * a if lstm else None, ldh, ph + 2 * a, ldh,
                    pg + 2 * ag if pg else None, ldp)
        _rec_steps(fn1, fn2, "hvk_lstm_step_fwd", (code, B, H), dirs, T, step,
                   _s(x))
        if save is not None:
            save["xg"] = xg_[:, :, :W]
            if lstm:
                save["gates"] = g_[:, :, :W]
    else:
        xf, wf = x.float(), w.float()
        xg = xf.reshape(B * T, I) @ wf[:, :I].t()
        if bias is not None:
            xg = xg + bias.float().view(1, -1)
        xg = xg.view(B, T, W)
        h_all = _rec_buf(st, "h", (B, T, DH), torch.float32, dev)
        if lstm:
            c_all = _rec_buf(st, "c", (B, T, DH), torch.float32, dev)
            gates = _rec_buf(st, "gates", (B, T, W), torch.float32, dev)
        for d, rev in dirs:
            wh = wf[d * gh:(d + 1) * gh, I:]
            h = torch.zeros(B, H)
            c = torch.zeros(B, H)
            for s in range(T):
                t = T - 1 - s if rev else s
                pre = xg[:, t, d * gh:(d + 1) * gh]
                if s:
                    pre = pre + h @ wh.t()
                if lstm:
                    gi = torch.sigmoid(pre[:, :H])
                    gf = torch.sigmoid(pre[:, H:2 * H])
                    gg = torch.tanh(pre[:, 2 * H:3 * H])
                    go = torch.sigmoid(pre[:, 3 * H:])
                    c = gf * c + gi * gg
                    h = go * torch.tanh(c)
                    c_all[:, t, d * H:(d + 1) * H] = c
                    gates[:, t, d * gh:(d + 1) * gh] = \
                        torch.cat((gi, gf, gg, go), 1)
                else:
                    h = torch.tanh(pre)
                h_all[:, t, d * H:(d + 1) * H] = h
        if save is not None:
            save["xg"] = xg
    if return_sequences:
        return h_all
    return _rec_last(h_all, dirs, H, T, out)


def lstm_bwd(err, x, w, save, dw, dbias, *, cell="lstm", accumulate="overwrite",
             need_err_input=True, err_input=None, direction="forward"):
    """Backward of lstm_fwd from its ``save`` dict, with its ``direction``.

    ``err`` is dL/dh_t for every step [B][T][D*H] (the layer ran with
    ``return_sequences``), or [B][D*H] = the error of the final states
    [h^f_{T-1} | h^r_0]: the block of a forward chain enters at t = T-1, that
    of a reverse chain at t = 0.  T step launches walk every chain from its
    end (forward chain t = T-1 .. 0, reverse chain t = 0 .. T-1; "both": one
    paired launch per step) and fill save["dg"] = dL/d(pre-activations)
    [B][T][D*NG*H] (and save["dc"] [T][B][D*H] float32 on the GPU); then
    ``dw[:, :I]`` (+)= dG^T.X with ``dbias`` (+)= its column sums, the rows
    of direction d of ``dw[:, I:]`` (+)= dG_d^T.Hprev_d over all B*T rows
    (Hprev_f[t] = h^f_{t-1}, Hprev_r[t] = h^r_{t+1}, zero at the chain's first
    step; ``accumulate``: True adds, "overwrite" writes, as in ``gemm``), and,
    with ``need_err_input``, err_input [B][T][I] = sum_d dG_d.Wx_d is
    returned: ONE GEMM over K = D*NG*H, no atomic accumulation.  ``dw`` is
    float32 [D*NG*H][I+H], ``dbias`` float32 [D*NG*H] or None, both
    direction-major as ``w`` and ``bias``.  Bit-reproducible under
    ``set_deterministic(True)``."""
    name = "lstm_bwd"
    dirs = _directions(name, direction)
    D = len(dirs)
    if cell not in _CELLS:
        raise ValueError("%s: unknown cell %r (lstm, rnn)" % (name, cell))
    ng = _CELLS[cell][1]
    if w.dim() != 2 or w.shape[0] % (D * ng):
        raise ValueError("%s: weights %s" % (name, tuple(w.shape)))
    B, T, I, H, code, ng = _lstm_args(name, x, w, None,
                                      w.shape[0] // (D * ng), cell, D)
    dev = x.device
    gh = ng * H
    W, DH = D * gh, D * H
    lstm = ng == 4
    seq = _rec_grad_check(name, accumulate, err, dw, dbias, B, T, DH, W,
                          I + H, W, dev)
    hdt = torch.bfloat16 if _gpu(x) else torch.float32
    need = [("h", (B, T, DH), hdt)]
    if lstm:
        need += [("c", (B, T, DH), torch.float32), ("gates", (B, T, W), hdt)]
    _rec_save_check(name, "lstm_fwd", save, need, dev)
    if need_err_input:
        _rec_err_input_check(name, err_input, B, T, I, hdt, dev)
    h_all = save["h"]
    if _gpu(x):
        if err.dtype != torch.bfloat16:
            raise TypeError("%s: GPU err must be bfloat16, got %s" %
                            (name, err.dtype))
        fn1 = _rec_fn("hvk_lstm_step_bwd")
        fn2 = _rec_fn("hvk_lstm_step_bwd2") if D == 2 else None
        P, PW = _r8(gh), _r8(W)
        if lstm:
            g_ = _rec_gates_check(name, "lstm_fwd", save, (B, T, PW))
        # Wh^T of every direction, one copy per call: the product of a step
        # sums over Wh's rows
        wt = _rec_buf(save, "_wht", (D, H, P), torch.bfloat16, dev)
        for d, _ in dirs:
            wt[d, :, :gh].copy_(w[d * gh:(d + 1) * gh, I:].t())
        dg_ = _rec_buf(save, "_dg", (B, T, PW), torch.bfloat16, dev,
                       zero=True)
        # dc[t] = dL/dc of the chain's previous step as step t leaves it
        dc = _rec_buf(save, "dc", (T, B, DH), torch.float32, dev) \
            if lstm else None
        pdg, pdc = dg_.data_ptr(), _p(dc)
        pwt = [wt.data_ptr() + 2 * d * H * P for d in range(D)]
        # what the step reads as "gates": the saved gates, RNN: h itself
        pgt, ldg = (g_.data_ptr(), T * PW) if lstm else \
            (h_all.data_ptr(), T * DH)
        pc = save["c"].data_ptr() if lstm else None
        pe, lde, se = err.data_ptr(), err.stride(0), \
            err.stride(1) if seq else 0
        ldh, ldp, BDH = T * DH, T * PW, B * DH

        def step(d, rev, s):
            t = s if rev else T - 1 - s
            k = 1 if rev else -1      # towards the chain's previous step
            oh = d * H
            a, ag, ac = t * DH + oh, t * PW + d * gh, t * BDH + oh
            if seq:
                e = pe + 2 * (t * se + oh)
            else:
                e = None if s else pe + 2 * oh
            # the step done one launch earlier is at t - k
            return (pdg + 2 * (ag - k * PW) if s else None, ldp, pwt[d], P,
                    e, lde, pgt + 2 * (ag if lstm else a), ldg,
                    pc + 4 * (a + k * DH) if lstm and s < T - 1 else None,
                    ldh, pc + 4 * a if lstm else None, ldh,
                    pdc + 4 * (ac - k * BDH) if lstm and s else None, DH,
                    pdc + 4 * ac if lstm else None, DH, pdg + 2 * ag, ldp)
        _rec_steps(fn1, fn2, "hvk_lstm_step_bwd", (code, B, H), dirs, T, step,
                   _s(x))
        dg = dg_[:, :, :W]
        dg2 = dg_.view(B * T, PW)[:, :W]
    else:
        dg = _rec_buf(save, "dg", (B, T, W), torch.float32, dev)
        ef = err.float()
        for d, rev in dirs:
            wh = w.float()[d * gh:(d + 1) * gh, I:]
            hs, gs = slice(d * H, (d + 1) * H), slice(d * gh, (d + 1) * gh)
            dc = torch.zeros(B, H)
            for s in range(T):
                t = s if rev else T - 1 - s
                tn = t - 1 if rev else t + 1
                tp = t + 1 if rev else t - 1
                dh = ef[:, t, hs] if seq else (ef[:, hs] if s == 0 else
                                               torch.zeros(B, H))
                if s:
                    dh = dh + dg[:, tn, gs] @ wh
                if lstm:
                    gi, gf, gg, go = save["gates"][:, t, gs].float() \
                        .split(H, 1)
                    tc = torch.tanh(save["c"][:, t, hs])
                    cp = save["c"][:, tp, hs] if s < T - 1 else \
                        torch.zeros(B, H)
                    dc = dc + dh * go * (1.0 - tc * tc)
                    dg[:, t, gs] = torch.cat((dc * gg * gi * (1.0 - gi),
                                              dc * cp * gf * (1.0 - gf),
                                              dc * gi * (1.0 - gg * gg),
                                              dh * tc * go * (1.0 - go)), 1)
                    dc = dc * gf
                else:
                    ht = h_all[:, t, hs].float()
                    dg[:, t, gs] = dh * (1.0 - ht * ht)
        dg2 = dg.view(B * T, W)
    save["dg"] = dg
    hp = _rec_hprev(save, h_all, dirs, B, T, H).view(B * T, DH)
    gemm(dg2, _rows(x, B, T), trans_a=True, out=dw[:, :I],
         accumulate=accumulate, bias_grad=dbias)
    for d, _ in dirs:
        gemm(dg2[:, d * gh:(d + 1) * gh], hp[:, d * H:(d + 1) * H],
             trans_a=True, out=dw[d * gh:(d + 1) * gh, I:],
             accumulate=accumulate)
    return _rec_err_input(err_input, dg2, w, B, T, I, hdt, dev) \
        if need_err_input else None


# GRU (docs/OPS.md "GRU"): gate order r, z, n; the reset gate multiplies the
# hidden-side product only, so it has step kernels and entry points of its own.
def gru_fwd(x, w, bias, H, *, return_sequences=False, save=None, out=None,
            ws=None, direction="forward"):
    """Forward of a GRU layer over ``x`` [B][T][I] (batch-major).

    ``direction`` ("forward", "reverse", "both"), D, the direction-major
    layout, the returned tensor and ``out`` are those of ``lstm_fwd``.  ``w``
    [D*3H][I+H]: per direction ONE parameter, ``w[:, :I]`` is Wx, ``w[:, I:]``
    is Wh, gate order r, z, n; ``bias`` [D*4H] = (b_r, b_z, b_n, b_hn) per
    direction, or None (torch: bias_ih = the block's [:3H], bias_hh = (0, 0,
    its [3H:])).  h starts at zero; h_{t-1} is the chain's previous step.

        r = sigmoid(x_t.Wxr^T + b_r + h_{t-1}.Whr^T)
        z = sigmoid(x_t.Wxz^T + b_z + h_{t-1}.Whz^T)
        hn = h_{t-1}.Whn^T + b_hn,  n = tanh(x_t.Wxn^T + b_n + r hn)
        h_t = (1 - z) n + z h_{t-1}

    One GEMM per direction (the [4H] bias blocks are not contiguous over the
    directions) projects all B*T rows with the block's bias[:3H] (float32
    ``xg``), then T step launches run on the current stream with no host
    synchronisation (capturable), paired for "both".  ``save`` (a dict)
    receives "h" [B][T][D*H], "hf" (h in float32: the carry z h_{t-1} is not
    rounded to bf16), "hn" float32, "gates" [B][T][D*3H] (post-activation r,
    z, n) and "xg" for gru_bwd, direction d of an axis of width D*W at
    ``[..., d*W:(d+1)*W]``; with ``save=None`` the gates are not written.  A
    kept ``save`` / ``ws`` dict is reused: no allocation from the second call
    on."""
    name = "gru_fwd"
    dirs = _directions(name, direction)
    D = len(dirs)
    B, T, I, H = _gru_args(name, x, w, bias, H, D)
    dev = x.device
    st = save if save is not None else (ws if ws is not None else {})
    gh = 3 * H
    W, DH = D * gh, D * H
    if not return_sequences:
        _rec_out_check(name, out, B, DH, dev)
    if _gpu(x):
        fn1 = _rec_fn("hvk_gru_step_fwd")
        fn2 = _rec_fn("hvk_gru_step_fwd2") if D == 2 else None
        PW = _r8(W)
        xg_ = _rec_buf(st, "_xg", (B, T, PW), torch.float32, dev)
        h_all = _rec_buf(st, "h", (B, T, DH), torch.bfloat16, dev)
        hf = _rec_buf(st, "hf", (B, T, DH), torch.float32, dev)
        hn = _rec_buf(st, "hn", (B, T, DH), torch.float32, dev)
        g_ = _rec_buf(st, "_gates", (B, T, PW), torch.bfloat16, dev) \
            if save is not None else None
        for d, _ in dirs:
            gemm(_rows(x, B, T), w[d * gh:(d + 1) * gh, :I], trans_b=True,
                 bias=None if bias is None else
                 bias[d * 4 * H:d * 4 * H + gh],
                 out=xg_.view(B * T, PW)[:, d * gh:(d + 1) * gh])
        ph, phf, phn = h_all.data_ptr(), hf.data_ptr(), hn.data_ptr()
        pxg, pg = xg_.data_ptr(), _p(g_)
        ldw, ldh, ldp = w.stride(0), T * DH, T * PW
        pw = [w.data_ptr() + 2 * (I + d * gh * ldw) for d in range(D)]
        pb = [None if bias is None else bias.data_ptr() + 4 * (d * 4 * H + gh)
              for d in range(D)]

        def step(d, rev, s):
            t = T - 1 - s if rev else s
            a, ag = t * DH + d * H, t * PW + d * gh     # row t of direction d
            ap = a + DH if rev else a - DH              # the chain's previous
            return (ph + 2 * ap if s else None, ldh, pw[d], ldw,
                    pxg + 4 * ag, ldp, phf + 4 * ap if s else None, ldh,
                    phf + 4 * a, ldh, phn + 4 * a, ldh, ph + 2 * a, ldh,
                    pg + 2 * ag if pg else None, ldp, pb[d])
        _rec_steps(fn1, fn2, "hvk_gru_step_fwd", (B, H), dirs, T, step, _s(x))
        if save is not None:
            save["xg"] = xg_[:, :, :W]
            save["gates"] = g_[:, :, :W]
    else:
        xf, wf = x.float(), w.float()
        xg = (xf.reshape(B * T, I) @ wf[:, :I].t()).view(B, T, W)
        if bias is not None:
            bf = bias.float().view(D, 4 * H)
            xg = xg + bf[:, :gh].reshape(1, 1, W)
        h_all = _rec_buf(st, "h", (B, T, DH), torch.float32, dev)
        gs = save if save is not None else {}   # kept for a backward only
        hn_all = _rec_buf(gs, "hn", (B, T, DH), torch.float32, dev)
        gates = _rec_buf(gs, "gates", (B, T, W), torch.float32, dev)
        for d, rev in dirs:
            wh = wf[d * gh:(d + 1) * gh, I:]
            bhn = torch.zeros(H) if bias is None else bf[d, gh:]
            h = torch.zeros(B, H)
            for s in range(T):
                t = T - 1 - s if rev else s
                xt = xg[:, t, d * gh:(d + 1) * gh]
                hh = h @ wh.t() if s else torch.zeros(B, gh)
                gr = torch.sigmoid(xt[:, :H] + hh[:, :H])
                gz = torch.sigmoid(xt[:, H:2 * H] + hh[:, H:2 * H])
                hn = hh[:, 2 * H:] + bhn
                gn = torch.tanh(xt[:, 2 * H:] + gr * hn)
                h = (1.0 - gz) * gn + gz * h
                h_all[:, t, d * H:(d + 1) * H] = h
                hn_all[:, t, d * H:(d + 1) * H] = hn
                gates[:, t, d * gh:(d + 1) * gh] = torch.cat((gr, gz, gn), 1)
        st["hf"] = h_all    # float32 already: one tensor serves both
        if save is not None:
            save["xg"] = xg
    if return_sequences:
        return h_all
    return _rec_last(h_all, dirs, H, T, out)


def gru_bwd(err, x, w, save, dw, dbias, *, accumulate="overwrite",
            need_err_input=True, err_input=None, direction="forward"):
    """Backward of gru_fwd from its ``save`` dict, with its ``direction``.

    ``err``, the walk of every chain from its end, Hprev_d, ``accumulate``
    and the direction-major ``dw`` [D*3H][I+H] are those of ``lstm_bwd``.  A
    step, with "next" the step done one launch earlier (t + 1 on a forward
    chain, t - 1 on a reverse one):

        dh = err_t + dGh_next.Wh + dcarry_next
        dn = dh (1 - z)(1 - n^2),  dz = dh (h_{t-1} - n) z(1 - z)
        dr = dn hn r(1 - r)
        dGx_t = (dr, dz, dn),  dGh_t = (dr, dz, dn r),  dcarry_t = dh z

    The steps fill save["dgx"] and save["dgh"] (two [B][T][D*3H] buffers: the
    gradient of the input-side and of the hidden-side pre-activations) and
    save["dcarry"] [T][B][D*H] float32; then, per direction d, its rows of
    ``dw[:, :I]`` (+)= dGx_d^T.X with the [:3H] of its ``dbias`` block (+)=
    the column sums, its rows of ``dw[:, I:]`` (+)= dGh_d^T.Hprev_d with the
    [3H:] of its ``dbias`` block (+)= the column sums of dGh_d's n block,
    and, with ``need_err_input``, err_input [B][T][I] = sum_d dGx_d.Wx_d (one
    GEMM) is returned.  ``dbias`` is float32 [D*4H] or None.
    Bit-reproducible under ``set_deterministic(True)``."""
    name = "gru_bwd"
    dirs = _directions(name, direction)
    D = len(dirs)
    if w.dim() != 2 or w.shape[0] % (3 * D):
        raise ValueError("%s: weights %s" % (name, tuple(w.shape)))
    B, T, I, H = _gru_args(name, x, w, None, w.shape[0] // (3 * D), D)
    dev = x.device
    gh = 3 * H
    W, DH = D * gh, D * H
    seq = _rec_grad_check(name, accumulate, err, dw, dbias, B, T, DH, W,
                          I + H, D * 4 * H, dev)
    hdt = torch.bfloat16 if _gpu(x) else torch.float32
    _rec_save_check(name, "gru_fwd", save,
                    (("h", (B, T, DH), hdt), ("hf", (B, T, DH), torch.float32),
                     ("hn", (B, T, DH), torch.float32),
                     ("gates", (B, T, W), hdt)), dev)
    if need_err_input:
        _rec_err_input_check(name, err_input, B, T, I, hdt, dev)
    h_all = save["h"]
    if _gpu(x):
        if err.dtype != torch.bfloat16:
            raise TypeError("%s: GPU err must be bfloat16, got %s" %
                            (name, err.dtype))
        fn1 = _rec_fn("hvk_gru_step_bwd")
        fn2 = _rec_fn("hvk_gru_step_bwd2") if D == 2 else None
        P, PW = _r8(gh), _r8(W)
        g_ = _rec_gates_check(name, "gru_fwd", save, (B, T, PW))
        # Wh^T of every direction, one copy per call: the product of a step
        # sums over Wh's rows
        wt = _rec_buf(save, "_wht", (D, H, P), torch.bfloat16, dev)
        for d, _ in dirs:
            wt[d, :, :gh].copy_(w[d * gh:(d + 1) * gh, I:].t())
        dgx_ = _rec_buf(save, "_dgx", (B, T, PW), torch.bfloat16, dev,
                        zero=True)
        dgh_ = _rec_buf(save, "_dgh", (B, T, PW), torch.bfloat16, dev,
                        zero=True)
        # dcarry[t] = dh_t z_t as step t leaves it (read by the chain's
        # previous step)
        dc = _rec_buf(save, "dcarry", (T, B, DH), torch.float32, dev)
        pdx, pdh, pdc = dgx_.data_ptr(), dgh_.data_ptr(), dc.data_ptr()
        pwt = [wt.data_ptr() + 2 * d * H * P for d in range(D)]
        pgt, phn = g_.data_ptr(), save["hn"].data_ptr()
        phf = save["hf"].data_ptr()
        pe, lde, se = err.data_ptr(), err.stride(0), \
            err.stride(1) if seq else 0
        ldh, ldp, BDH = T * DH, T * PW, B * DH

        def step(d, rev, s):
            t = s if rev else T - 1 - s
            k = 1 if rev else -1      # towards the chain's previous step
            oh = d * H
            a, ag, ac = t * DH + oh, t * PW + d * gh, t * BDH + oh
            if seq:
                e = pe + 2 * (t * se + oh)
            else:
                e = None if s else pe + 2 * oh
            # the step done one launch earlier is at t - k
            return (pdh + 2 * (ag - k * PW) if s else None, ldp, pwt[d], P,
                    e, lde, pgt + 2 * ag, ldp, phn + 4 * a, ldh,
                    phf + 4 * (a + k * DH) if s < T - 1 else None, ldh,
                    pdc + 4 * (ac - k * BDH) if s else None, DH,
                    pdc + 4 * ac, DH, pdx + 2 * ag, ldp, pdh + 2 * ag, ldp)
        _rec_steps(fn1, fn2, "hvk_gru_step_bwd", (B, H), dirs, T, step, _s(x))
        dgx, dgh = dgx_[:, :, :W], dgh_[:, :, :W]
        dgx2 = dgx_.view(B * T, PW)[:, :W]
        dgh2 = dgh_.view(B * T, PW)[:, :W]
    else:
        dgx = _rec_buf(save, "dgx", (B, T, W), torch.float32, dev)
        dgh = _rec_buf(save, "dgh", (B, T, W), torch.float32, dev)
        dc = _rec_buf(save, "dcarry", (T, B, DH), torch.float32, dev)
        ef = err.float()
        zero = torch.zeros(B, H)
        for d, rev in dirs:
            wh = w.float()[d * gh:(d + 1) * gh, I:]
            hs, gs = slice(d * H, (d + 1) * H), slice(d * gh, (d + 1) * gh)
            for s in range(T):
                t = s if rev else T - 1 - s
                tn = t - 1 if rev else t + 1
                tp = t + 1 if rev else t - 1
                dh = ef[:, t, hs] if seq else (ef[:, hs] if s == 0 else zero)
                if s:
                    dh = dh + dgh[:, tn, gs] @ wh + dc[tn][:, hs]
                gr, gz, gn = save["gates"][:, t, gs].float().split(H, 1)
                hp = save["hf"][:, tp, hs] if s < T - 1 else zero
                dn = dh * (1.0 - gz) * (1.0 - gn * gn)
                dz = dh * (hp - gn) * gz * (1.0 - gz)
                dr = dn * save["hn"][:, t, hs] * gr * (1.0 - gr)
                dgx[:, t, gs] = torch.cat((dr, dz, dn), 1)
                dgh[:, t, gs] = torch.cat((dr, dz, dn * gr), 1)
                dc[t][:, hs] = dh * gz
        dgx2, dgh2 = dgx.view(B * T, W), dgh.view(B * T, W)
    save["dgx"], save["dgh"] = dgx, dgh
    hp = _rec_hprev(save, h_all, dirs, B, T, H).view(B * T, DH)
    sums = None
    if dbias is not None:
        sums = _rec_buf(save, "_dbh", (D, gh), torch.float32, dev)
        if accumulate is True:
            sums.zero_()
    for d, _ in dirs:
        gs = slice(d * gh, (d + 1) * gh)
        b0 = d * 4 * H
        gemm(dgx2[:, gs], _rows(x, B, T), trans_a=True, out=dw[gs, :I],
             accumulate=accumulate,
             bias_grad=None if dbias is None else dbias[b0:b0 + gh])
        # the ones column of the hidden-side GEMM sums every column of dGh;
        # its n block is the gradient of b_hn
        gemm(dgh2[:, gs], hp[:, d * H:(d + 1) * H], trans_a=True,
             out=dw[gs, I:], accumulate=accumulate,
             bias_grad=None if sums is None else sums[d])
        if dbias is not None:
            if accumulate is True:
                dbias[b0 + gh:b0 + 4 * H] += sums[d, 2 * H:]
            else:
                dbias[b0 + gh:b0 + 4 * H].copy_(sums[d, 2 * H:])
    return _rec_err_input(err_input, dgx2, w, B, T, I, hdt, dev) \
        if need_err_input else None

# ------------------------------------------- restricted Boltzmann machines
# docs/OPS.md "Restricted Boltzmann machines"; kernels in csrc/kernels/rbm.hip.
def _rbm_fn(name):
    fn = getattr(_lib.lib(), name, None)
    if fn is None:
        raise _lib.KernelLibraryMissing(
            "%s lacks %s - rebuild with python -m veles_amd.ops.build" %
            (_lib.LIB_PATH, name))
    return fn


def rbm_layout(V, H):
    """(offset of hbias, offset of vbias, length) of the flat float32 buffer
    [W [H][V] | hbias [H] | vbias [V]]: every segment starts on a 16-element
    boundary."""
    V, H = int(V), int(H)
    hb = -(-(H * V) // 16) * 16
    vb = hb + -(-H // 16) * 16
    return hb, vb, vb + -(-V // 16) * 16


def rbm_uniforms(rows, N, seed, base=0, device="cpu"):
    """The float32 uniforms [rows][N] of one sampling call: element (b, j) is
    (hash32(base + b N + j, seed) >> 8) 2^-24, indices modulo 2^32."""
    i = (torch.arange(rows * N, dtype=torch.int64, device=device) +
         (int(base) & 0xFFFFFFFF)) & 0xFFFFFFFF
    u = (_hash32(i, int(seed) & 0xFFFFFFFF) >> 8).float() / 16777216.0
    return u.view(rows, N)


def _rbm_mat(name, what, t, rows, cols, dev, gpu):
    """A [rows][cols] operand with contiguous rows and one row pitch."""
    if not isinstance(t, torch.Tensor) or t.dim() != 2:
        raise ValueError("%s: %s must be a 2-D tensor" % (name, what))
    if (rows is not None and t.shape[0] != rows) or t.shape[1] != cols:
        raise ValueError("%s: %s must be [%s][%d], got %s" % (
            name, what, "rows" if rows is None else rows, cols,
            tuple(t.shape)))
    if t.device != dev:
        raise ValueError("%s: %s on %s, weights on %s" % (name, what,
                                                         t.device, dev))
    if t.stride(1) != 1 or (t.shape[0] > 1 and t.stride(0) < cols):
        raise ValueError("%s: %s rows must be contiguous (strides %s)" %
                         (name, what, t.stride()))
    if gpu:
        if t.dtype != torch.bfloat16:
            raise TypeError("%s: GPU %s must be bfloat16, got %s" %
                            (name, what, t.dtype))
    elif not t.is_floating_point():
        raise TypeError("%s: %s must be floating-point, got %s" %
                        (name, what, t.dtype))
    ld = t.stride(0) if t.shape[0] > 1 else max(cols, t.stride(0))
    if t.shape[0] * ld >= 1 << 31:
        raise ValueError("%s: %s %d x %d exceeds 2^31 elements" %
                         (name, what, t.shape[0], ld))
    return ld


def rbm_sample(x, w, bias, *, transposed=False, n=None, probs=None,
               sample=None, seed=0, seed_dev=None, base=0):
    """One half of a Gibbs step from the weights ``w`` [H][V]:

        transposed=False: x [rows][V] -> p = sigmoid(x . w^T + bias) [rows][H]
        transposed=True:  x [rows][H] -> p = sigmoid(x . w   + bias) [rows][V]

    (the same ``w``: no transposed copy exists), ``probs`` = p and ``sample``
    = 1 where u < p else 0, with the uniform of element (b, j) of the
    [rows][N] output u = (hash32(base + b N + j, seed) >> 8) 2^-24
    (:func:`rbm_uniforms`) compared in float32 before any bfloat16 rounding.
    Only the first ``n`` rows are read and written.  Either output may be
    None, not both.  ``seed_dev`` (int32 [1] on the device) replaces
    ``seed``.  GPU: x, w, probs, sample bfloat16, bias float32; one launch,
    no synchronisation.  Returns (probs, sample)."""
    name = "rbm_sample"
    if not isinstance(w, torch.Tensor) or w.dim() != 2 or min(w.shape) < 1:
        raise ValueError("%s: weights must be [H][V]" % name)
    gpu = _gpu(w)
    dev = w.device
    H, V = w.shape
    K, U = (H, V) if transposed else (V, H)
    ldw = _rbm_mat(name, "weights", w, H, V, dev, gpu)
    if not isinstance(x, torch.Tensor) or x.dim() != 2 or x.shape[0] < 1:
        raise ValueError("%s: input must be [rows][%d]" % (name, K))
    rows = x.shape[0]
    ldx = _rbm_mat(name, "input", x, rows, K, dev, gpu)
    if probs is None and sample is None:
        raise ValueError("%s: neither probs nor sample is wanted" % name)
    ldp = lds = 0
    if probs is not None:
        ldp = _rbm_mat(name, "probs", probs, rows, U, dev, gpu)
    if sample is not None:
        lds = _rbm_mat(name, "sample", sample, rows, U, dev, gpu)
    if not isinstance(bias, torch.Tensor) or tuple(bias.shape) != (U,) or \
            not bias.is_contiguous() or bias.device != dev:
        raise ValueError("%s: bias must be a contiguous [%d] on %s" %
                         (name, U, dev))
    if gpu and bias.dtype != torch.float32:
        raise TypeError("%s: GPU bias must be float32, got %s" %
                        (name, bias.dtype))
    if not bias.is_floating_point():
        raise TypeError("%s: bias must be floating-point" % name)
    n = rows if n is None else int(n)
    if n < 1 or n > rows:
        raise ValueError("%s: %d valid rows of %d" % (name, n, rows))
    base = int(base)
    if base < 0:
        raise ValueError("%s: base %d" % (name, base))
    if seed_dev is not None and (
            not isinstance(seed_dev, torch.Tensor) or
            seed_dev.dtype != torch.int32 or seed_dev.numel() != 1 or
            seed_dev.device != dev):
        raise ValueError("%s: seed_dev must be an int32 [1] on %s" %
                         (name, dev))
    if gpu:
        _lib.check(_rbm_fn("hvk_rbm_sample")(
            1 if transposed else 0, n, V, H, _p(x), ldx, _p(w), ldw,
            _p(bias), _p(probs), ldp, _p(sample), lds,
            int(seed) & 0xFFFFFFFF, _p(seed_dev), base & 0xFFFFFFFF, _s(w)),
            "hvk_rbm_sample")
        return probs, sample
    if seed_dev is not None:
        seed = int(seed_dev.reshape(-1)[0]) & 0xFFFFFFFF
    xf, wf = x[:n].float(), w.float()
    pre = (xf @ wf if transposed else xf @ wf.t()) + bias.float().view(1, -1)
    p = 1.0 / (1.0 + torch.exp(-pre))
    if probs is not None:
        probs[:n] = p.to(probs.dtype)
    if sample is not None:
        u = rbm_uniforms(n, U, seed, base)
        sample[:n] = (u < p).to(sample.dtype)
    return probs, sample


def rbm_grad(v0, h0, vk, hk, grad, *, n=None, scale=None, splits=0):
    """The contrastive-divergence statistic over the first ``n`` rows,
    OVERWRITING the flat float32 buffer ``grad`` (:func:`rbm_layout`):

        W     = scale (h0^T . v0 - hk^T . vk)          [H][V]
        hbias = scale sum_b (h0 - hk),  vbias = scale sum_b (v0 - vk)

    ``scale`` defaults to -1/n (the gradient a descent step subtracts); the
    padding between the segments is set to 0.  v0 / vk are [rows][V], h0 / hk
    [rows][H] (bfloat16 on the GPU).  ``splits`` forces the number of batch
    slices on the GPU (0: chosen); the slices are added in order, so the
    result does not depend on scheduling."""
    name = "rbm_grad"
    for what, t in (("v0", v0), ("h0", h0), ("vk", vk), ("hk", hk),
                    ("grad", grad)):
        if not isinstance(t, torch.Tensor):
            raise TypeError("%s: %s must be a tensor" % (name, what))
    if v0.dim() != 2 or h0.dim() != 2 or min(v0.shape) < 1 or \
            min(h0.shape) < 1:
        raise ValueError("%s: v0 must be [rows][V], h0 [rows][H]" % name)
    rows, V = v0.shape
    H = h0.shape[1]
    gpu = _gpu(grad)
    dev = grad.device
    ld_v0 = _rbm_mat(name, "v0", v0, rows, V, dev, gpu)
    ld_h0 = _rbm_mat(name, "h0", h0, rows, H, dev, gpu)
    ld_vk = _rbm_mat(name, "vk", vk, rows, V, dev, gpu)
    ld_hk = _rbm_mat(name, "hk", hk, rows, H, dev, gpu)
    off_hb, off_vb, total = rbm_layout(V, H)
    if grad.dtype != torch.float32:
        raise TypeError("%s: grad must be float32, got %s" %
                        (name, grad.dtype))
    if grad.dim() != 1 or grad.numel() != total or not grad.is_contiguous():
        raise ValueError("%s: grad must be a contiguous flat [%d] (V %d, H "
                         "%d), got %s" % (name, total, V, H,
                                          tuple(grad.shape)))
    if H * V >= 1 << 31:
        raise ValueError("%s: %d x %d weights exceed 2^31 elements" %
                         (name, H, V))
    n = rows if n is None else int(n)
    if n < 1 or n > rows:
        raise ValueError("%s: %d valid rows of %d" % (name, n, rows))
    splits = int(splits)
    if splits < 0:
        raise ValueError("%s: splits %d" % (name, splits))
    scale = -1.0 / n if scale is None else float(scale)
    if gpu:
        sp = _rbm_fn("hvk_rbm_grad_splits")(n, V, H, splits)
        if sp < 1 or sp > 65535:
            raise ValueError("%s: %d splits for %d rows" % (name, splits, n))
        ws = None if sp == 1 else _grow_ws("rbm_grad", sp * total,
                                           torch.float32, dev)
        _lib.check(_rbm_fn("hvk_rbm_grad")(
            n, V, H, _p(v0), ld_v0, _p(h0), ld_h0, _p(vk), ld_vk, _p(hk),
            ld_hk, _p(grad), scale, _p(ws), sp, _s(grad)), "hvk_rbm_grad")
        return grad
    a0, b0 = h0[:n].float(), v0[:n].float()
    ak, bk = hk[:n].float(), vk[:n].float()
    grad.zero_()
    grad[:H * V] = (scale * (a0.t() @ b0 - ak.t() @ bk)).reshape(-1)
    grad[off_hb:off_hb + H] = scale * (a0 - ak).sum(0)
    grad[off_vb:off_vb + V] = scale * (b0 - bk).sum(0)
    return grad


# ------------------------------------------------------------ self-attention
# docs/OPS.md "Attention".  Head widths the kernels are built for, and the
# rows a workgroup owns / sweeps per tile (csrc/kernels/attention.hip).
ATTN_HEAD_DIMS = (32, 64, 128)
ATTN_TQ = 128
ATTN_TK = 32


def _attn_fn(name):
    fn = getattr(_lib.lib(), name, None)
    if fn is None:
        raise _lib.KernelLibraryMissing(
            "%s lacks %s - rebuild with python -m veles_amd.ops.build" %
            (_lib.LIB_PATH, name))
    return fn


def attn_head_dim(E, heads, name="attention"):
    """D = E / heads, checked against the supported head widths (the same
    check on every device, so a config that runs on the CPU runs on the GPU)"""
    E, heads = int(E), int(heads)
    if heads < 1 or E < 1 or E % heads:
        raise ValueError("%s: width %d does not split into %d heads" %
                         (name, E, heads))
    D = E // heads
    if D not in ATTN_HEAD_DIMS:
        raise ValueError("%s: head width %d (= %d / %d heads) is not "
                         "supported; supported head widths are %s" %
                         (name, D, E, heads, list(ATTN_HEAD_DIMS)))
    return D


def _attn_view(name, what, t, like=None):
    """(B, T, E, pitch) of a [B][T][E] view with contiguous rows and one row
    pitch over [B][T]"""
    if not isinstance(t, torch.Tensor):
        raise TypeError("%s: %s must be a tensor, got %s" % (
            name, what, type(t).__name__))
    if t.dim() != 3 or min(t.shape) < 1:
        raise ValueError("%s: %s must be [B][T][E], got %s" %
                         (name, what, tuple(t.shape)))
    B, T, E = t.shape
    ld = t.stride(1) if B * T > 1 else max(t.stride(1), E)
    if t.stride(2) != 1 or ld < E or (B > 1 and t.stride(0) != T * ld):
        raise ValueError("%s: %s rows must be contiguous with one pitch over "
                         "[B][T] (strides %s)" % (name, what, t.stride()))
    if B * T * ld >= 1 << 31:
        raise ValueError("%s: %s spans %d x %d x %d elements, the limit is "
                         "2^31 - 1" % (name, what, B, T, ld))
    if like is not None:
        if tuple(t.shape) != tuple(like.shape):
            raise ValueError("%s: %s is %s, q is %s" % (
                name, what, tuple(t.shape), tuple(like.shape)))
        if t.dtype != like.dtype:
            raise TypeError("%s: %s is %s, q is %s" % (
                name, what, t.dtype, like.dtype))
        if t.device != like.device:
            raise ValueError("%s: %s is on %s, q on %s" % (
                name, what, t.device, like.device))
    return B, T, E, ld


def _attn_dtype(name, q):
    if _gpu(q):
        if q.dtype != torch.bfloat16:
            raise TypeError("%s: GPU operands must be bfloat16, got %s" %
                            (name, q.dtype))
        if q.data_ptr() % 2:
            raise ValueError("%s: operands off the element grid" % name)
    elif q.dtype != torch.float32:
        raise TypeError("%s: CPU operands must be float32, got %s" %
                        (name, q.dtype))


def _attn_stat(name, what, t, B, NH, T, dev):
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or \
            tuple(t.shape) != (B, NH, T) or not t.is_contiguous() or \
            t.device != dev:
        raise ValueError("%s: %s must be a contiguous float32 [%d][%d][%d] "
                         "on %s" % (name, what, B, NH, T, dev))


def _attn_heads(t, NH, D):
    """[B][T][NH*D] -> [B][NH][T][D] view"""
    B, T, _ = t.shape
    return t.reshape(B, T, NH, D).permute(0, 2, 1, 3)


def _attn_mask(T, dev):
    """True where key j is hidden from query i (j > i)"""
    i = torch.arange(T, device=dev)
    return i.view(1, T) > i.view(T, 1)


def attention_fwd(q, k, v, heads, causal=False, out=None, save=None):
    """Scaled dot-product self-attention over ``heads`` heads.

    ``q``, ``k``, ``v`` are [B][T][E] views with contiguous rows and a row
    pitch each (column slices of one fused projection buffer need no copy);
    head h is columns h*D .. (h+1)*D - 1, D = E / heads in (32, 64, 128).
    Per (batch, head): S = q k^T / sqrt(D); with ``causal`` key j is visible
    to query i iff j <= i; P = softmax_j(S); o = P v.  Returns o [B][T][E]
    (``out`` when given); ``save`` (a dict) receives "lse" = ln sum_j
    exp(S_ij), float32 [B][heads][T], for :func:`attention_bwd`.

    GPU: bfloat16 operands, ``hvk_attn_fwd`` (flash style: no [T][T] tensor
    in memory) on the current stream.  CPU: float32, S materialised per
    (batch, head) with the row maximum subtracted."""
    name = "attention_fwd"
    B, T, E, ldq = _attn_view(name, "q", q)
    _attn_dtype(name, q)
    _, _, _, ldk = _attn_view(name, "k", k, like=q)
    _, _, _, ldv = _attn_view(name, "v", v, like=q)
    NH = int(heads)
    D = attn_head_dim(E, NH, name)
    dev = q.device
    if out is None:
        out = torch.empty(B, T, E, dtype=q.dtype, device=dev)
    _, _, _, ldo = _attn_view(name, "out", out, like=q)
    save = {} if save is None else save
    lse = _rec_buf(save, "lse", (B, NH, T), torch.float32, dev)
    if _gpu(q):
        _lib.check(_attn_fn("hvk_attn_fwd")(
            _p(q), ldq, _p(k), ldk, _p(v), ldv, _p(out), ldo, _p(lse), B, T,
            NH, D, int(bool(causal)), _s(q)), "hvk_attn_fwd")
        return out
    qh, kh, vh = (_attn_heads(t, NH, D) for t in (q, k, v))
    s = (qh @ kh.transpose(2, 3)) * (1.0 / math.sqrt(D))
    if causal:
        s = s.masked_fill(_attn_mask(T, dev), float("-inf"))
    m = s.max(dim=3, keepdim=True).values
    e = torch.exp(s - m)
    l = e.sum(dim=3, keepdim=True)
    lse.copy_((m + torch.log(l)).squeeze(3))
    o = (e / l) @ vh
    out.copy_(o.permute(0, 2, 1, 3).reshape(B, T, E))
    return out


def attention_bwd(do, q, k, v, o, save, heads, causal=False, dq=None,
                  dk=None, dv=None, ws=None):
    """Backward of :func:`attention_fwd` from its ``save`` ("lse"): returns
    (dq, dk, dv), each [B][T][E] (the given views, e.g. column slices of one
    fused gradient buffer, or new tensors).

        P = exp(S - lse),  dV = P^T dO,  dP = dO V^T,
        delta = rowsum(dO * O),  dS = P * (dP - delta) / sqrt(D),
        dQ = dS K,  dK = dS^T Q

    GPU: ``hvk_attn_bwd_delta``, ``hvk_attn_bwd_dkv`` and ``hvk_attn_bwd_dq``
    (P recomputed from lse in both; no atomics, the result repeats bit for
    bit); ``ws`` (a dict) keeps "delta".  CPU: float32."""
    name = "attention_bwd"
    B, T, E, ldq = _attn_view(name, "q", q)
    _attn_dtype(name, q)
    _, _, _, ldk = _attn_view(name, "k", k, like=q)
    _, _, _, ldv = _attn_view(name, "v", v, like=q)
    _, _, _, ldo = _attn_view(name, "o", o, like=q)
    _, _, _, lddo = _attn_view(name, "do", do, like=q)
    NH = int(heads)
    D = attn_head_dim(E, NH, name)
    dev = q.device
    if not isinstance(save, dict) or "lse" not in save:
        raise ValueError("%s: save must be attention_fwd's dict" % name)
    lse = save["lse"]
    _attn_stat(name, "save[\"lse\"]", lse, B, NH, T, dev)
    grads = []
    for what, t in (("dq", dq), ("dk", dk), ("dv", dv)):
        if t is None:
            t = torch.empty(B, T, E, dtype=q.dtype, device=dev)
        grads.append((t, _attn_view(name, what, t, like=q)[3]))
    (dq, lddq), (dk, lddk), (dv, lddv) = grads
    ws = {} if ws is None else ws
    delta = _rec_buf(ws, "delta", (B, NH, T), torch.float32, dev)
    c = int(bool(causal))
    if _gpu(q):
        s = _s(q)
        _lib.check(_attn_fn("hvk_attn_bwd_delta")(
            _p(do), lddo, _p(o), ldo, _p(delta), B, T, NH, D, s),
            "hvk_attn_bwd_delta")
        _lib.check(_attn_fn("hvk_attn_bwd_dkv")(
            _p(q), ldq, _p(k), ldk, _p(v), ldv, _p(do), lddo, _p(lse),
            _p(delta), _p(dk), lddk, _p(dv), lddv, B, T, NH, D, c, s),
            "hvk_attn_bwd_dkv")
        _lib.check(_attn_fn("hvk_attn_bwd_dq")(
            _p(q), ldq, _p(k), ldk, _p(v), ldv, _p(do), lddo, _p(lse),
            _p(delta), _p(dq), lddq, B, T, NH, D, c, s), "hvk_attn_bwd_dq")
        return dq, dk, dv
    scale = 1.0 / math.sqrt(D)
    qh, kh, vh, oh, doh = (_attn_heads(t, NH, D) for t in (q, k, v, o, do))
    s = (qh @ kh.transpose(2, 3)) * scale
    p = torch.exp(s - lse.unsqueeze(3))
    if causal:
        p = p.masked_fill(_attn_mask(T, dev), 0.0)
    delta.copy_((doh * oh).sum(3))
    dp = doh @ vh.transpose(2, 3)
    ds = p * (dp - delta.unsqueeze(3)) * scale
    for t, g in ((dq, ds @ kh), (dk, ds.transpose(2, 3) @ qh),
                 (dv, p.transpose(2, 3) @ doh)):
        t.copy_(g.permute(0, 2, 1, 3).reshape(B, T, E))
    return dq, dk, dv


def _mha_args(name, x, w_in, w_out, bias, heads):
    """Shared host checks of mha_fwd / mha_bwd; returns (B, T, I, E, D)"""
    for what, t in (("x", x), ("w_in", w_in), ("w_out", w_out)):
        if not isinstance(t, torch.Tensor):
            raise TypeError("%s: %s must be a tensor, got %s" % (
                name, what, type(t).__name__))
    if x.dim() != 3 or min(x.shape) < 1:
        raise ValueError("%s: input must be [B][T][I], got %s" %
                         (name, tuple(x.shape)))
    B, T, I = x.shape
    if w_out.dim() != 2 or w_out.shape[0] != w_out.shape[1]:
        raise ValueError("%s: w_out must be [E][E], got %s" %
                         (name, tuple(w_out.shape)))
    E = w_out.shape[0]
    D = attn_head_dim(E, heads, name)
    if w_in.dim() != 2 or tuple(w_in.shape) != (3 * E, I):
        raise ValueError("%s: w_in must be [%d][%d] (rows q, k, v; E = %d, "
                         "I = %d), got %s" % (name, 3 * E, I, E, I,
                                              tuple(w_in.shape)))
    if w_in.device != x.device or w_out.device != x.device or \
            (bias is not None and bias.device != x.device):
        raise ValueError("%s: operands on different devices" % name)
    if x.stride(2) != 1 or (B * T > 1 and x.stride(1) < I) or \
            (B > 1 and x.stride(0) != T * x.stride(1)) or \
            w_in.stride(1) != 1 or w_out.stride(1) != 1:
        raise ValueError("%s: input rows must be contiguous with one pitch "
                         "over [B][T], weight rows contiguous (strides %s, "
                         "%s, %s)" % (name, x.stride(), w_in.stride(),
                                      w_out.stride()))
    if bias is not None and (tuple(bias.shape) != (4 * E,) or
                             not bias.is_contiguous()):
        raise ValueError("%s: bias must be a contiguous [%d] = (b_q, b_k, "
                         "b_v, b_o), got %s" % (name, 4 * E,
                                                tuple(bias.shape)))
    if _gpu(x):
        if x.dtype != torch.bfloat16 or w_in.dtype != torch.bfloat16 or \
                w_out.dtype != torch.bfloat16:
            raise TypeError("%s: GPU input and weights must be bfloat16, got "
                            "%s / %s / %s" % (name, x.dtype, w_in.dtype,
                                              w_out.dtype))
        if bias is not None and bias.dtype != torch.float32:
            raise TypeError("%s: GPU bias must be float32, got %s" %
                            (name, bias.dtype))
    elif not (x.is_floating_point() and w_in.is_floating_point() and
              w_out.is_floating_point()):
        raise TypeError("%s: floating-point operands, got %s / %s / %s" %
                        (name, x.dtype, w_in.dtype, w_out.dtype))
    if B * T * max(3 * E, x.stride(1) if B * T > 1 else I) >= 1 << 31:
        raise ValueError("%s: %d x %d x %d exceeds 2^31 elements" %
                         (name, B, T, max(3 * E, I)))
    return B, T, I, E, D


def _mha_rows(x, B, T):
    return x.as_strided((B * T, x.shape[2]),
                        (x.stride(1) if B * T > 1 else x.shape[2], 1))


def mha_fwd(x, w_in, w_out, bias, heads, *, causal=False, save=None,
            ws=None, out=None):
    """Multi-head self-attention layer over ``x`` [B][T][I] (batch-major):
    ``torch.nn.MultiheadAttention(E, heads, bias=True, batch_first=True)``
    applied to (x, x, x).

        qkv = x w_in^T + bias[:3E]      w_in [3E][I], rows q, k, v, each
                                        block head-major
        o   = attention(q, k, v)        :func:`attention_fwd`
        y   = o w_out^T + bias[3E:]     w_out [E][E]

    ``bias`` is [4E] or None.  Returns y [B][T][E] (``out`` when given).
    ``save`` (a dict) receives "qkv" [B*T][3E], "o" [B][T][E] and "lse" for
    :func:`mha_bwd`; q, k and v are column slices of "qkv": no head
    transposes, no copies.  A kept ``save`` / ``ws`` dict is reused: no
    allocation from the second call on."""
    name = "mha_fwd"
    B, T, I, E, D = _mha_args(name, x, w_in, w_out, bias, heads)
    dev = x.device
    st = save if save is not None else (ws if ws is not None else {})
    dt = torch.bfloat16 if _gpu(x) else torch.float32
    if out is not None and (tuple(out.shape) != (B, T, E) or
                            not out.is_contiguous() or out.device != dev or
                            out.dtype != dt):
        raise ValueError("%s: out must be a contiguous %s [%d][%d][%d] on %s"
                         % (name, dt, B, T, E, dev))
    if out is None:
        out = torch.empty(B, T, E, dtype=dt, device=dev)
    qkv = _rec_buf(st, "qkv", (B * T, 3 * E), dt, dev)
    o = _rec_buf(st, "o", (B, T, E), dt, dev)
    b_in = None if bias is None else bias[:3 * E]
    b_out = None if bias is None else bias[3 * E:]
    x2 = _mha_rows(x, B, T)
    if _gpu(x):
        gemm(x2, w_in, trans_b=True, bias=b_in, out=qkv)
    else:
        r = x2.float() @ w_in.float().t()
        qkv.copy_(r if b_in is None else r + b_in.float())
    q3 = qkv.view(B, T, 3 * E)
    attention_fwd(q3[:, :, :E], q3[:, :, E:2 * E], q3[:, :, 2 * E:], heads,
                  causal=causal, out=o, save=st)
    if _gpu(x):
        gemm(o.view(B * T, E), w_out, trans_b=True, bias=b_out,
             out=out.view(B * T, E))
    else:
        r = o.view(B * T, E) @ w_out.float().t()
        out.view(B * T, E).copy_(r if b_out is None else r + b_out.float())
    return out


def mha_bwd(err, x, w_in, w_out, save, dw_in, dw_out, dbias, heads, *,
            causal=False, accumulate="overwrite", need_err_input=True,
            err_input=None, aux=None, aux_act=0):
    """Backward of :func:`mha_fwd` from its ``save`` dict.  ``err`` is dL/dy
    [B][T][E].

        dw_out (+)= err^T o, dbias[3E:] (+)= its column sums (one GEMM)
        do = err w_out;  (dq | dk | dv) = attention_bwd, into one fused
        [B*T][3E] buffer save["dqkv"]
        dw_in (+)= dqkv^T x, dbias[:3E] (+)= its column sums
        err_input [B][T][I] = dqkv w_in, times f'(aux) of the layer below
        when ``aux_act`` is set (the GEMM's epilogue)

    ``dw_in`` float32 [3E][I], ``dw_out`` float32 [E][E], ``dbias`` float32
    [4E] or None; ``accumulate``: True adds, "overwrite" writes, as in
    ``gemm``.  Returns err_input (None without ``need_err_input``)."""
    name = "mha_bwd"
    B, T, I, E, D = _mha_args(name, x, w_in, w_out, None, heads)
    dev = x.device
    gpu = _gpu(x)
    dt = torch.bfloat16 if gpu else torch.float32
    if accumulate not in (True, "overwrite"):
        raise ValueError("%s: accumulate must be True or \"overwrite\"" %
                         name)
    if not isinstance(err, torch.Tensor) or \
            tuple(err.shape) != (B, T, E) or not err.is_contiguous() or \
            err.device != dev:
        raise ValueError("%s: err must be a contiguous [%d][%d][%d] on %s" %
                         (name, B, T, E, dev))
    if gpu and err.dtype != torch.bfloat16:
        raise TypeError("%s: GPU err must be bfloat16, got %s" %
                        (name, err.dtype))
    for what, t, shape in (("dw_in", dw_in, (3 * E, I)),
                           ("dw_out", dw_out, (E, E))):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or \
                tuple(t.shape) != shape or not t.is_contiguous() or \
                t.device != dev:
            raise ValueError("%s: %s must be a contiguous float32 [%d][%d] "
                             "on %s" % (name, what, shape[0], shape[1], dev))
    if dbias is not None and (dbias.dtype != torch.float32 or
                              tuple(dbias.shape) != (4 * E,) or
                              not dbias.is_contiguous() or
                              dbias.device != dev):
        raise ValueError("%s: dbias must be a contiguous float32 [%d] on %s"
                         % (name, 4 * E, dev))
    NH = int(heads)
    _rec_save_check(name, "mha_fwd", save,
                    (("qkv", (B * T, 3 * E), dt), ("o", (B, T, E), dt),
                     ("lse", (B, NH, T), torch.float32)), dev)
    aux_act = act_code(aux_act)
    if aux_act and aux is None:
        raise ValueError("%s: aux_act without aux" % name)
    if need_err_input:
        _rec_err_input_check(name, err_input, B, T, I, dt, dev)
        if aux_act and (aux.numel() != B * T * I or not aux.is_contiguous()):
            raise ValueError("%s: aux must be a contiguous [%d][%d][%d]" %
                             (name, B, T, I))
    err2 = err.view(B * T, E) if gpu else err.float().view(B * T, E)
    o2 = save["o"].view(B * T, E)
    x2 = _mha_rows(x, B, T) if gpu else _mha_rows(x, B, T).float()
    wi, wo = (w_in, w_out) if gpu else (w_in.float(), w_out.float())
    db_in = None if dbias is None else dbias[:3 * E]
    db_out = None if dbias is None else dbias[3 * E:]
    gemm(err2, o2, trans_a=True, out=dw_out, accumulate=accumulate,
         bias_grad=db_out)
    do = _rec_buf(save, "do", (B, T, E), dt, dev)
    gemm(err2, wo, out=do.view(B * T, E))
    dqkv = _rec_buf(save, "dqkv", (B * T, 3 * E), dt, dev)
    q3, g3 = save["qkv"].view(B, T, 3 * E), dqkv.view(B, T, 3 * E)
    attention_bwd(do, q3[:, :, :E], q3[:, :, E:2 * E], q3[:, :, 2 * E:],
                  save["o"], save, heads, causal=causal, dq=g3[:, :, :E],
                  dk=g3[:, :, E:2 * E], dv=g3[:, :, 2 * E:], ws=save)
    gemm(dqkv, x2, trans_a=True, out=dw_in, accumulate=accumulate,
         bias_grad=db_in)
    if not need_err_input:
        return None
    if err_input is None:
        err_input = torch.empty(B, T, I, dtype=dt, device=dev)
    gemm(dqkv, wi, out=err_input.view(B * T, I),
         aux=aux.reshape(B * T, I) if aux_act else None, aux_act=aux_act)
    return err_input


# ------------------------------------------------ position-wise feed-forward
FFN_ACT = {"gelu": 0, "gelu_tanh": 1, "str": 2}
_FFN_C = 0.7978845608028654       # sqrt(2 / pi)
_FFN_K = 0.044715

# du^T of ffn_bwd's NN weight gradient: True, the tile path of
# hvk_ffn_act_bwd (one pass, 8 B per element); False, the plain backward and
# then transpose_colsum (10 B per element).  Same bits either way; a
# measuring switch for tools/bench_ffn.py and the tests.
_FFN_TILE = True


def set_ffn_tile(on):
    """Switch ``ffn_bwd``'s du^T between the tile path (True, the default)
    and plain backward + ``transpose_colsum``; returns the old value."""
    global _FFN_TILE
    old, _FFN_TILE = _FFN_TILE, bool(on)
    return old


def ffn_act_code(act):
    try:
        return FFN_ACT[act]
    except (KeyError, TypeError):
        raise ValueError("ffn: unknown activation %r (one of %s)" % (
            act, ", ".join(sorted(FFN_ACT)))) from None


def ffn_partials(P, F, transposed):
    """Slabs per column of ``hvk_ffn_act_bwd``'s column sums over [P][F]: a
    function of the shape and of whether du^T is written only."""
    g = _bn_fn("hvk_ffn_act_partials")(int(P), int(F), int(bool(transposed)))
    if g < 1:
        raise ValueError("ffn: no grid for P = %d, F = %d, transposed = %s" %
                         (P, F, transposed))
    return g


def ffn_act_ref(u, act):
    """a(u) in ``u``'s own floating-point type (the CPU path, float32)"""
    code = ffn_act_code(act)
    if code == 0:
        return 0.5 * u * (1.0 + torch.erf(u * (0.5 ** 0.5)))
    if code == 1:
        return 0.5 * u * (1.0 + torch.tanh(
            _FFN_C * (u + _FFN_K * u * u * u)))
    return torch.where(u > 0, u, torch.zeros_like(u))


def ffn_dact_ref(u, act):
    """a'(u), from the pre-activation"""
    code = ffn_act_code(act)
    if code == 0:
        return 0.5 * (1.0 + torch.erf(u * (0.5 ** 0.5))) + \
            u * torch.exp(-0.5 * u * u) * 0.3989422804014327
    if code == 1:
        t = torch.tanh(_FFN_C * (u + _FFN_K * u * u * u))
        return 0.5 * (1.0 + t) + 0.5 * u * (1.0 - t * t) * \
            (_FFN_C * (1.0 + 3.0 * _FFN_K * u * u))
    return (u > 0).to(u.dtype)


def ffn_act_fwd(u, act="gelu", out=None):
    """h = a(u) over a tensor whose last axis has contiguous elements (any
    contiguous shape, or 2-D rows with a pitch).  ``out`` may be ``u``.
    GPU: bf16, ``hvk_ffn_act_fwd`` (float32 inside); CPU: float32."""
    name = "ffn_act_fwd"
    code = ffn_act_code(act)
    P, F_, ldu = _bn_rows(name, "u", u)
    _bn_xdtype(name, u)
    if out is None:
        out = torch.empty(u.shape, dtype=u.dtype, device=u.device)
    _, _, ldh = _bn_rows(name, "out", out, like=u)
    if _gpu(u):
        _lib.check(_bn_fn("hvk_ffn_act_fwd")(
            _p(u), ldu, _p(out), ldh, P, F_, code, _s(u)), "hvk_ffn_act_fwd")
        return out
    out.copy_(ffn_act_ref(u, act))
    return out


def ffn_act_bwd(dh, u, act="gelu", *, out=None, out_t=None, db1=None,
                accumulate="overwrite", ws=None):
    """du = dh a'(u) (``out``, which may be ``dh``); ``out_t`` [F][P], when
    given, gets du^T; ``db1`` float32 [F], when given, gets (``"overwrite"``)
    or is added (True) the column sums of the STORED du.  GPU: bf16,
    ``hvk_ffn_act_bwd``: one pass plus the ordered finish, the tile path when
    ``out_t`` is given (P and F multiples of 64); ``ws`` (a dict) keeps the
    slab workspace.  CPU: float32."""
    name = "ffn_act_bwd"
    code = ffn_act_code(act)
    P, F_, ldu = _bn_rows(name, "u", u)
    _bn_xdtype(name, u)
    _, _, lddh = _bn_rows(name, "dh", dh, like=u)
    if accumulate not in (True, "overwrite"):
        raise ValueError("%s: accumulate must be True or \"overwrite\"" %
                         name)
    if out is None:
        out = torch.empty(u.shape, dtype=u.dtype, device=u.device)
    _, _, lddu = _bn_rows(name, "out", out, like=u)
    if db1 is not None:
        _bn_vecs(name, F_, u, db1=db1)
    lddut = P
    if out_t is not None:
        if not isinstance(out_t, torch.Tensor) or \
                tuple(out_t.shape) != (F_, P) or out_t.dtype != u.dtype or \
                out_t.device != u.device or out_t.stride(1) != 1 or \
                (F_ > 1 and out_t.stride(0) < P):
            raise ValueError("%s: out_t must be a %s [%d][%d] with contiguous "
                             "rows on %s" % (name, u.dtype, F_, P, u.device))
        lddut = out_t.stride(0) if F_ > 1 else P
        if _gpu(u) and (P % 64 or F_ % 64):
            raise ValueError("%s: out_t needs P and F multiples of 64, got "
                             "%d x %d" % (name, P, F_))
    if _gpu(u):
        ws = {} if ws is None else ws
        G = ffn_partials(P, F_, out_t is not None)
        w = _rec_buf(ws, "act_bwd", (F_ * G,), torch.float32, u.device)
        _lib.check(_bn_fn("hvk_ffn_act_bwd")(
            _p(dh), lddh, _p(u), ldu, _p(out), lddu, _p(out_t), lddut, P, F_,
            code, _p(db1), int(accumulate is True), _p(w), _s(u)),
            "hvk_ffn_act_bwd")
        return out
    out.copy_(dh * ffn_dact_ref(u, act))
    if out_t is not None:
        out_t.copy_(out.reshape(P, F_).t())
    if db1 is not None:
        s = _bn_chain_sum(out.reshape(P, F_))
        if accumulate is True:
            db1.add_(s)
        else:
            db1.copy_(s)
    return out


def _ffn_args(name, x, w1, w2, bias):
    """Shared host checks of ffn_fwd / ffn_bwd; returns (P, I, F, E, ldx)"""
    for what, t in (("w1", w1), ("w2", w2)):
        if not isinstance(t, torch.Tensor):
            raise TypeError("%s: %s must be a tensor, got %s" % (
                name, what, type(t).__name__))
    P, I, ldx = _bn_rows(name, "x", x)
    _bn_xdtype(name, x)
    if w1.dim() != 2 or w1.shape[1] != I or w1.shape[0] < 1:
        raise ValueError("%s: w1 must be [F][%d] (I = %d), got %s" % (
            name, I, I, tuple(w1.shape)))
    F_ = w1.shape[0]
    if w2.dim() != 2 or w2.shape[1] != F_ or w2.shape[0] < 1:
        raise ValueError("%s: w2 must be [E][%d] (F = %d), got %s" % (
            name, F_, F_, tuple(w2.shape)))
    E = w2.shape[0]
    if w1.stride(1) != 1 or w2.stride(1) != 1:
        raise ValueError("%s: weight rows must be contiguous (strides %s, %s)"
                         % (name, w1.stride(), w2.stride()))
    if w1.device != x.device or w2.device != x.device or \
            (bias is not None and bias.device != x.device):
        raise ValueError("%s: operands on different devices" % name)
    if w1.dtype != x.dtype or w2.dtype != x.dtype:
        raise TypeError("%s: weights must be %s as x, got %s / %s" % (
            name, x.dtype, w1.dtype, w2.dtype))
    if bias is not None and (bias.dtype != torch.float32 or
                             tuple(bias.shape) != (F_ + E,) or
                             not bias.is_contiguous()):
        raise ValueError("%s: bias must be a contiguous float32 [%d] = (b1, "
                         "b2), got %s %s" % (name, F_ + E, bias.dtype,
                                             tuple(bias.shape)))
    if P * max(F_, E, ldx) >= 1 << 31:
        raise ValueError("%s: %d x %d exceeds 2^31 - 1 elements" % (
            name, P, max(F_, E, ldx)))
    return P, I, F_, E, ldx


def _ffn_wgrad_nn(g, a):
    """GradientDescent.run's rule for an FC weight gradient g^T a"""
    from veles_amd.models.gd import _wgrad_nn
    return _wgrad_nn(g, a)


def ffn_fwd(x, w1, w2, bias, act="gelu", *, save=None, out=None, ws=None):
    """Position-wise feed-forward layer over the last axis of ``x`` (every
    other axis is a row): float64 ``Sequential(Linear(I, F), GELU(),
    Linear(F, E))`` is the reference.

        u = x w1^T + bias[:F]      w1 [F][I]
        h = a(u)                   :func:`ffn_act_fwd`
        y = h w2^T + bias[F:]      w2 [E][F]

    ``bias`` is [F + E] or None; both biases ride the GEMM epilogues.
    Returns y, ``x``'s shape with E for I (``out`` when given).  ``save`` (a
    dict) receives "u" and "h" [P][F] for :func:`ffn_bwd`; without it
    (evaluation) h overwrites u, which lives in ``ws``.  A kept dict is
    reused: no allocation from the second call on."""
    name = "ffn_fwd"
    ffn_act_code(act)
    P, I, F_, E, ldx = _ffn_args(name, x, w1, w2, bias)
    dev, dt = x.device, x.dtype
    oshape = tuple(x.shape[:-1]) + (E,)
    if out is not None and (tuple(out.shape) != oshape or
                            not out.is_contiguous() or out.device != dev or
                            out.dtype != dt):
        raise ValueError("%s: out must be a contiguous %s %s on %s" %
                         (name, dt, oshape, dev))
    if out is None:
        out = torch.empty(oshape, dtype=dt, device=dev)
    st = save if save is not None else (ws if ws is not None else {})
    u = _rec_buf(st, "u", (P, F_), dt, dev)
    h = _rec_buf(st, "h", (P, F_), dt, dev) if save is not None else u
    b1 = None if bias is None else bias[:F_]
    b2 = None if bias is None else bias[F_:]
    x2 = x.as_strided((P, I), (ldx, 1))
    gemm(x2, w1, trans_b=True, bias=b1, out=u)
    ffn_act_fwd(u, act, out=h)
    gemm(h, w2, trans_b=True, bias=b2, out=out.view(P, E))
    return out


def ffn_bwd(err, x, w1, w2, save, dw1, dw2, dbias, act="gelu", *,
            accumulate="overwrite", need_err_input=True, err_input=None,
            aux=None, aux_act=0):
    """Backward of :func:`ffn_fwd` from its ``save`` dict; ``err`` is dL/dy.

        dbias[F:] (+)= sum_P err,  dw2 (+)= err^T h,  dh = err w2
        du = dh a'(u), rounded to the storage type, in dh's buffer
        dbias[:F] (+)= sum_P du (of the stored du),  dw1 (+)= du^T x
        err_input = du w1, times f'(aux) of the layer below when ``aux_act``
        is set (the GEMM's epilogue)

    A weight gradient goes the way ``GradientDescent.run`` sends an FC one:
    transpose + NN GEMM where its rule allows (err^T and dbias[F:] from
    ``transpose_colsum``; du^T from the activation kernel's tile path, see
    :func:`set_ffn_tile`), else the TN GEMM.  ``dw1`` float32 [F][I], ``dw2``
    float32 [E][F], ``dbias`` float32 [F + E] or None; ``accumulate``: True
    adds, "overwrite" writes.  ``save`` also keeps "dh" (= du), "dut", "dyt"
    and the workspaces.  Returns err_input (None without
    ``need_err_input``)."""
    name = "ffn_bwd"
    ffn_act_code(act)
    P, I, F_, E, ldx = _ffn_args(name, x, w1, w2, None)
    dev, dt = x.device, x.dtype
    if accumulate not in (True, "overwrite"):
        raise ValueError("%s: accumulate must be True or \"overwrite\"" %
                         name)
    oshape = tuple(x.shape[:-1]) + (E,)
    if not isinstance(err, torch.Tensor) or tuple(err.shape) != oshape or \
            not err.is_contiguous() or err.device != dev or err.dtype != dt:
        raise ValueError("%s: err must be a contiguous %s %s on %s" %
                         (name, dt, oshape, dev))
    for what, t, shape in (("dw1", dw1, (F_, I)), ("dw2", dw2, (E, F_))):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or \
                tuple(t.shape) != shape or not t.is_contiguous() or \
                t.device != dev:
            raise ValueError("%s: %s must be a contiguous float32 [%d][%d] "
                             "on %s" % (name, what, shape[0], shape[1], dev))
    if dbias is not None and (not isinstance(dbias, torch.Tensor) or
                              dbias.dtype != torch.float32 or
                              tuple(dbias.shape) != (F_ + E,) or
                              not dbias.is_contiguous() or
                              dbias.device != dev):
        raise ValueError("%s: dbias must be a contiguous float32 [%d] on %s"
                         % (name, F_ + E, dev))
    _rec_save_check(name, "ffn_fwd", save,
                    (("u", (P, F_), dt), ("h", (P, F_), dt)), dev)
    aux_act = act_code(aux_act)
    if aux_act and aux is None:
        raise ValueError("%s: aux_act without aux" % name)
    if need_err_input:
        if err_input is not None and (
                tuple(err_input.shape) != tuple(x.shape) or
                not err_input.is_contiguous() or err_input.device != dev or
                err_input.dtype != dt):
            raise ValueError("%s: err_input must be a contiguous %s %s" %
                             (name, dt, tuple(x.shape)))
        if aux_act and (aux.numel() != P * I or not aux.is_contiguous()):
            raise ValueError("%s: aux must be a contiguous %s" %
                             (name, tuple(x.shape)))
    add = accumulate is True
    g2 = err.view(P, E)
    x2 = x.as_strided((P, I), (ldx, 1))
    u, h = save["u"], save["h"]
    db1 = None if dbias is None else dbias[:F_]
    db2 = None if dbias is None else dbias[F_:]
    if _ffn_wgrad_nn(g2, h):
        gt = _rec_buf(save, "dyt", (E, P), dt, dev)
        gws = _rec_buf(save, "dyt_ws", (P // 64 * E,), torch.float32, dev)
        transpose_colsum(g2, out=gt, colsum=db2, accumulate=add, ws=gws)
        gemm(gt, h, out=dw2, accumulate=accumulate)
    else:
        gemm(g2, h, trans_a=True, out=dw2, accumulate=accumulate,
             bias_grad=db2)
    dh = _rec_buf(save, "dh", (P, F_), dt, dev)
    gemm(g2, w2, out=dh)
    if _ffn_wgrad_nn(dh, x2):
        dut = _rec_buf(save, "dut", (F_, P), dt, dev)
        if _FFN_TILE:
            ffn_act_bwd(dh, u, act, out=dh, out_t=dut, db1=db1,
                        accumulate=accumulate, ws=save)
        else:
            ffn_act_bwd(dh, u, act, out=dh, ws=save)
            tws = _rec_buf(save, "dut_ws", (P // 64 * F_,), torch.float32,
                           dev)
            transpose_colsum(dh, out=dut, colsum=db1, accumulate=add, ws=tws)
        gemm(dut, x2, out=dw1, accumulate=accumulate)
    else:
        ffn_act_bwd(dh, u, act, out=dh, db1=db1, accumulate=accumulate,
                    ws=save)
        gemm(dh, x2, trans_a=True, out=dw1, accumulate=accumulate)
    if not need_err_input:
        return None
    if err_input is None:
        err_input = torch.empty(x.shape, dtype=dt, device=dev)
    gemm(dh, w1, out=err_input.view(P, I),
         aux=aux.reshape(P, I) if aux_act else None, aux_act=aux_act)
    return err_input
