"""Dropout on the attention weights (docs/OPS.md "Attention") on the float32
CPU path; tests/test_attention_dropout_gpu.py runs these helpers on the kernels.

Oracle: test_attention_ref.oracle's P, P~ = P o M inv (M the mask reference,
inv = 1 / (1 - p)), o = P~ v, dV = P~^T dO, dP = (dO V^T) o M inv, dS = P (dP -
rowsum(dO o)) / sqrt(D); lse unchanged.  Bounds: test_attention_ref's derivation
term by term with inv carried where the kernels multiply by it (ED = 4 u: the
float32 inv and its product): AO = P~ |v|; ADP becomes M inv ADP at gamma(D) +
ED; dV = inv sum_i M (h(P) + P (ePb + gamma(T) + ED)) |dO| (P is rounded to
bf16, the float32 sum scaled at the store); the statistics and dS see P.

Read-out: q = 0 makes P uniform over the n_i visible keys, so with one-hot v, k
and dO: o[i][j] = dv[j][i] = M_ij inv / n_i, the mask itself, held to half a bf16
ulp (GPU) plus F32T = 2^-22 + 4 u (ln T + 2) relative (lse, the exponential,
the difference, the scale); with v_j = dO_i = e_0 (dP~ = 1) dq[i][j] = (M_ij
inv - delta_i) / (n_i sqrt(D)), delta_i = dO_i . o_i of the o the backward is
given, held to half a bf16 ulp (GPU: dS is packed to bf16, one term per sum)
plus F32T (M inv + |delta|) / (n sqrt(D)); kept and dropped entries are a full
inv / (n_i sqrt(D)) apart."""
import math
import pickle

import numpy as np
import pytest
import torch

import veles_amd.ops as ops
from test_attention_ref import (BF_U, EXP_REL, TINY, heads_of, make_case,
                                oracle, unheads)
from test_attention_units import _layers, _state, _wf
from test_step_tail_ref import U, Ratios, bf_half_ulp, f64, gamma

ED = 4 * U
READOUT = [(T, D, c, r) for T, D in ((32, 32), (33, 64), (128, 128))
           for c in (False, True) for r in (0, 5)]
NAMES = ("o", "lse", "dq", "dk", "dv")


def keep_inv(B, NH, T, seed, p, base_row=0):
    inv = np.float32(1.0) / (np.float32(1.0) - np.float32(p))
    return ops.attention_dropout_mask_ref(B, NH, T, seed, p,
                                          base_row).numpy(), float(inv)


def check_drop(r, got, case, NH, causal, p, seed, gpu, tk=None):
    """got: o, lse, dq, dk, dv of a run at (p, seed) against the oracle, each
    element within its bound (the module docstring)"""
    arrs = [f64(t) for t in case]
    keep, inv = keep_inv(arrs[0].shape[0], NH, arrs[0].shape[1], seed, p)
    ref = oracle(*arrs, NH, causal)
    qh, kh, vh, doh = (heads_of(t, NH) for t in arrs)
    T, D = qh.shape[2], qh.shape[3]
    scale, km, P = 1.0 / math.sqrt(D), keep * inv, ref["P"]
    Pd, tr = P * km, lambda a: a.transpose(0, 1, 3, 2)
    oh = Pd @ vh
    dP, delta = (doh @ tr(vh)) * km, (doh * oh).sum(3, keepdims=True)
    dS = P * (dP - delta) * scale
    ref.update(o=unheads(oh), dq=unheads(dS @ kh), dk=unheads(tr(dS) @ qh),
               dv=unheads(tr(Pd) @ doh))
    qh, kh, vh, doh, dS = (np.abs(t) for t in (qh, kh, vh, doh, dS))
    A = np.einsum("bhid,bhjd->bhij", qh, kh) * scale
    R = A.max(3)
    es = gamma(D + 2) * A
    eP = es.max(3) + 2 * U * R + EXP_REL
    eR = (-(-T // tk) if gpu else 1) * (EXP_REL + 2 * U) + 2 * U * R
    eL = eP + gamma(T) + eR
    b_lse = eL + 4 * U * (R + math.log(T) + 1.0)

    def finish(b, val):
        return b + (bf_half_ulp(np.abs(val) + b) if gpu else 4 * U * np.abs(val))
    b_o = finish((Pd @ vh) * ((BF_U if gpu else 0.0) + eP + gamma(T) + eR +
                              eL + 4 * U + ED)[..., None] + TINY, oh)
    ePb = es + (b_lse + 2 * U * (2 * R + math.log(T)) + EXP_REL)[..., None]
    ed = (doh * b_o).sum(3) + gamma(D + 1) * (doh * np.abs(oh)).sum(3)
    ADP = np.einsum("bhid,bhjd->bhij", doh, vh) * km
    eds = P * scale * (ePb * np.abs(dP - delta) + (gamma(D) + ED) * ADP +
                       ed[..., None] + 3 * U * (np.abs(dP) + np.abs(delta)))
    edsr = eds + gamma(T) * dS + (bf_half_ulp(dS + eds) if gpu else 0.0)
    HP = bf_half_ulp(P * (1.0 + ePb)) if gpu else 0.0
    bd = {"o": b_o, "lse": b_lse,
          "dv": np.einsum("bhij,bhid->bhjd",
                          HP * km + Pd * (ePb + gamma(T) + ED), doh),
          "dk": np.einsum("bhij,bhid->bhjd", edsr, qh),
          "dq": np.einsum("bhij,bhjd->bhid", edsr, kh)}
    for n in NAMES:
        if n[0] == "d":
            bd[n] = finish(bd[n] + TINY, heads_of(ref[n], NH))
        r.see(n, np.abs(f64(got[n]) - ref[n]),
              bd[n] if n == "lse" else unheads(bd[n]))


def run_core(case, NH, causal, **kw):
    """forward + backward on the device and in the dtype of ``case``"""
    q, k, v, do = case
    save = {}
    o = ops.attention_fwd(q, k, v, NH, causal=causal, save=save, **kw)
    dq, dk, dv = ops.attention_bwd(do, q, k, v, o, save, NH, causal=causal,
                                   **kw)
    return {"o": o, "lse": save["lse"], "dq": dq, "dk": dk, "dv": dv}


def check_readout(T, D, causal, base_row, seed, gpu, run):
    """``run(case, **kw)`` -> run_core's dict at the caller's seed; 2 batch
    items x 3 heads at p = 0.5 (the module docstring)"""
    B, NH, p = 2, 3, 0.5

    def onehot(cols):
        x = torch.zeros(B, T, NH, D)
        x[:, torch.arange(T), :, cols] = 1.0
        return x.view(B, T, NH * D)
    q, ek, e0 = 0 * onehot(0), onehot(torch.arange(T)), onehot(0)
    vis = np.tril(np.ones((T, T), bool)) if causal else np.ones((T, T), bool)
    keep, inv = keep_inv(B, NH, T, seed, p, base_row)
    keep, n, kw = keep & vis, vis.sum(1)[:, None], dict(dropout=p,
                                                        base_row=base_row)
    f32t = 2.0 ** -22 + 4 * U * (math.log(T) + 2)
    got = run((q, ek, ek, ek), NH, causal, **kw)
    want = keep * inv / n
    tol = (bf_half_ulp(want) if gpu else 0.0) + f32t * want
    for name, m in (("o", heads_of(f64(got["o"]), NH)[..., :T]),
                    ("dv", heads_of(f64(got["dv"]), NH)[..., :T]
                     .transpose(0, 1, 3, 2))):
        assert np.array_equal(m != 0, keep), name
        assert (np.abs(m - want) <= tol).all(), name
    got = run((q, ek, e0, e0), NH, causal, **kw)
    delta = heads_of(f64(got["o"]), NH)[..., :1]          # dO_i = e_0
    want = np.where(vis, (keep * inv - delta) / (n * math.sqrt(D)), 0.0)
    f32t = f32t * (keep * inv + np.abs(delta)) / (n * math.sqrt(D))
    tol = f32t + (bf_half_ulp(np.abs(want) + f32t) if gpu else 0.0)
    dq = heads_of(f64(got["dq"]), NH)[..., :T]
    assert (np.abs(dq - want) <= tol).all(), np.abs(dq - want).max()


@pytest.mark.parametrize("T,D,causal,base_row", READOUT)
def test_cpu_mask_readout(T, D, causal, base_row):
    check_readout(T, D, causal, base_row, 77, False,
                  lambda *a, **kw: run_core(*a, seed=77, **kw))


@pytest.mark.parametrize("causal", (False, True))
def test_cpu_general_within_the_bound(causal):
    case = make_case(2, 33, 2, 64, seed=1)
    check_drop(Ratios(), run_core(case, 2, causal, dropout=0.1, seed=5), case,
               2, causal, 0.1, 5, False)
    for bad in (dict(dropout=1.0, seed=5), dict(dropout=0.1)):   # no seed
        with pytest.raises(ValueError):
            run_core(case, 2, causal, **bad)


def drop_layers():
    layers = _layers(heads=1, causal=True)
    layers[0]["->"]["dropout"] = 0.5
    return layers


def test_unit_drops_on_train_minibatches_only():
    from veles_amd.dummy import DummyLauncher
    from veles_amd.models import Attention
    with pytest.raises(ValueError):
        Attention(DummyLauncher(), output_sample_shape=64, dropout=1.0)
    wf = _wf(drop_layers())
    wf.run_steps(1)
    att = wf.forwards[0]
    w_in, w_out = att.split(att.weights_lp, att.n_in)

    def fwd(**kw):
        return ops.mha_fwd(att.input.devmem, w_in, w_out, att.bias_master, 1,
                           causal=True, **kw)
    plain = fwd()
    att.run()
    assert att.drop_ == {"dropout": 0.5, "base_row": 0, "seed": att.seed}
    assert not torch.equal(att.output.devmem, plain)
    assert torch.equal(att.output.devmem, fwd(**att.drop_))
    wf.loader.minibatch_class = 1                     # validation
    att.run()
    assert att.drop_ == {} and torch.equal(att.output.devmem, plain)
    wf.loader.minibatch_class, wf.testing = 2, True
    att.run()
    assert att.drop_ == {} and torch.equal(att.output.devmem, plain)


def check_resume(backend):
    """4 steps, pickle, unpickle, 3 steps draw the masks of 7 steps"""
    from veles_amd.backends import Device
    from veles_amd.dummy import DummyLauncher
    a = _wf(drop_layers(), backend)
    a.run_steps(7)          # one at a time: _wf reseeds the shared generator
    c = _wf(_layers(heads=1, causal=True), backend)
    c.run_steps(7)
    b = _wf(drop_layers(), backend)
    b.run_steps(4)
    b = pickle.loads(pickle.dumps(b, protocol=pickle.HIGHEST_PROTOCOL))
    b.workflow = DummyLauncher()
    b.initialize(device=Device(backend=backend))
    b.run_steps(3)
    assert b.forwards[0].drop_["dropout"] == 0.5
    assert torch.equal(_state(a), _state(b))
    assert not torch.equal(_state(a), _state(c))


def test_unit_snapshot_resumes_the_mask_stream():
    check_resume("cpu")
