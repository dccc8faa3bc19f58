"""Which launches the LayerNorm, BatchNorm / column-statistics, depthwise-convolution and attention entry points accept
and what they compute, at the smallest shapes that take each branch of their host-side launch code (csrc/dispatch.h and
the launchers of norm.hip, bn.hip, conv.hip, attention*.hip): every chunk count, flag, operand mode, kernel width, io
mode and head dimension an entry point tells apart, with the combinations it refuses.

The entry points are called through ``hip.lib()``, so a refusal is seen as its return code.  Every output is NaN before
the launch and has slack on both sides, which must still be NaN afterwards.  The return code must be the recorded one;
a refused launch leaves its outputs untouched; an accepted launch must match a float64 reference under the tolerance the
kernel's own test uses (test_layernorm_gpu.py, test_kernels_gpu.py, test_dwconv_any_k_gpu.py, test_conv_bn_bf16_gpu.py,
test_attention_gpu.py, test_attention_headdim_gpu.py, test_attention_bf16_storage_gpu.py) AND reproduce the recorded
SHA-256 prefix of its output bytes: the launch code may be reorganised, the kernels, grids and arguments it ends in may
not change.  Where a kernel writes bf16, the bound is the fp32 form's plus one bf16 rounding of the element (2^-8
relative, as test_conv_bn_bf16_gpu.py's ``bf16_close``), or equality with the fp32 form rounded once where the kernel's
test states that.

tests/golden/launch_dispatch.json is recorded on the GPU from the commit BEFORE a change to the launch code:
``python tests/test_launch_dispatch_gpu.py --record [path]`` (two passes; a digest that differs between them is dropped,
the return code and the float64 check stay).  The first-generation attention kernels at head dims 64 / 128 are only
reachable with FS2_ATTN_GEN1, which the library reads once per process: that group runs in a child process."""
import functools
import hashlib
import json
import math
import os
import subprocess
import sys
from pathlib import Path

import pytest
import torch
import torch.nn.functional as F

REPO = Path(__file__).resolve().parent.parent
if str(REPO) not in sys.path:
    sys.path.insert(0, str(REPO))

from fastspeech2_lightning_amd import hip as H  # noqa: E402
from tests import layernorm_references as R  # noqa: E402
from tests import test_layernorm_gpu as LN  # noqa: E402
from tests.test_dwconv_any_k_gpu import close  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = REPO / "tests" / "golden" / "launch_dispatch.json"
PAD = 1 << 12  # elements of slack on both sides of every device tensor
SEED, STEP_VALUE = (1 << 33) + 0x1234, 5
BF16_ULP = 2.0 ** -8  # one bf16 rounding of an element, relative (test_conv_bn_bf16_gpu.py: bf16_close)
f32, bf16, f64 = torch.float32, torch.bfloat16, torch.float64


def P(t):
    return None if t is None else t.data_ptr()


def lib():
    return H.lib(), H._stream()


def step():
    if "step" not in _CACHE:
        _CACHE["step"] = torch.full((1,), STEP_VALUE, dtype=torch.int64, device="cuda")
    return _CACHE["step"]


def factors(p, *shape):
    """the dropout factors of (p, SEED, step) at the linear element indices of a tensor of this shape"""
    return R.drop_factors(p, SEED, STEP_VALUE, math.prod(shape)).view(shape)


def dev(t):
    buf = torch.zeros(t.numel() + 2 * PAD, dtype=t.dtype, device="cuda")
    v = buf[PAD:PAD + t.numel()].view(t.shape)
    v.copy_(t)
    return v


class Outs:
    """The tensors one launch writes: NaN before it, slack on both sides.  ``scratch``: work space the caller hands in,
    whose contents are no result (not in the digest, not required to stay untouched by a refusal)."""

    def __init__(self):
        self.bufs, self.t = [], []

    def new(self, *shape, dtype=f32, scratch=False):
        n = math.prod(shape)
        buf = torch.full((n + 2 * PAD,), float("nan"), dtype=dtype, device="cuda")
        v = buf[PAD:PAD + n].view(shape)
        self.bufs.append((buf, n))
        if not scratch:
            self.t.append(v)
        return v

    def slack_untouched(self):
        return all(bool(torch.isnan(b[:PAD]).all()) and bool(torch.isnan(b[PAD + n:]).all()) for b, n in self.bufs)

    def untouched(self):
        return all(bool(torch.isnan(t).all()) for t in self.t)

    def digest(self):
        h = hashlib.sha256()
        for t in self.t:
            h.update(t.contiguous().view(-1).view(torch.uint8).cpu().numpy().tobytes())
        return h.hexdigest()[:12]


def near(got, ref, tol, what, floor_one=False, rounded=False):
    """max |got - ref| against tol * max |ref| (``floor_one``: of max(1, max |ref|)); ``rounded``: got is bf16 -- each
    element may also be off by one bf16 rounding of its reference"""
    got, ref = got.detach().float().cpu().double().reshape(ref.shape), ref.double()
    assert bool(torch.isfinite(got).all()), what
    scale = max(float(ref.abs().max()), 1.0 if floor_one else 1e-6)
    excess = (got - ref).abs() - (BF16_ULP * ref.abs() if rounded else 0.0)
    err = float(excess.max()) / scale
    print(f"{what}: err {err:.3e} tol {tol:.3e}")
    assert err < tol, f"{what}: err {err:.3e} > {tol:.3e}"


_CACHE = {}


def cached(fn):
    @functools.wraps(fn)
    def wrapper(*a):
        key = (fn.__name__,) + a
        if key not in _CACHE:
            _CACHE[key] = fn(*a)
        return _CACHE[key]
    return wrapper


# ---------------------------------------------------------------------------------------------------------------------
# LayerNorm: the seven entry points of norm.hip
# ---------------------------------------------------------------------------------------------------------------------
LN_SHAPES = [(5, 256), (5, 512), (5, 768), (5, 1024), (5, 1028), (5, 258), (4100, 256)]
DZ_SCALE = 0.7


@cached
def ln_case(M, C):
    """test_layernorm_gpu.py's case (inputs, float64 references, PyTorch's fp32 results as the yardstick) with device
    copies that have slack.  The saved statistics handed to the backward kernels are PyTorch's fp32 ones."""
    c = LN.Case(M, C, "randn")
    c.s = {k: dev(v) for k, v in (("x", c.x), ("gamma", c.gamma), ("beta", c.beta), ("dy", c.dy), ("add", c.add),
                                  ("dy_b", c.dy.bfloat16()), ("mean", c.mean32), ("rstd", c.rstd32))}
    c.yards = {}
    return c


def ln_yard(c, key, dy):
    if key not in c.yards:
        c.yards[key] = c.yard_bwd(dy)
    return c.yards[key]


def ln_fwd(M, C, entry, p=0.0):
    c, (L, s) = ln_case(M, C), lib()
    d, o = c.s, Outs()
    yb = entry == "fwd_b"
    y, mean, rstd = o.new(M, C, dtype=bf16 if yb else f32), o.new(M), o.new(M)
    a = (P(d["x"]), P(d["gamma"]), P(d["beta"]), P(y), P(mean), P(rstd), M, C, LN.EPS)
    if entry == "fwd_drop":
        rc = L.fs2hip_layernorm_fwd_drop(*a, p, SEED, P(step()), s)
    else:
        rc = getattr(L, "fs2hip_layernorm_" + entry)(*a, s)

    def check():
        fac = factors(p, M, C)
        y64 = c.y64 * fac.double()
        if yb:  # the fp32 entry point's result rounded once, its statistics unchanged (test_bf16_forward)
            _, o32, _ = ln_fwd(M, C, "fwd")
            assert torch.equal(y, o32.t[0].bfloat16()) and torch.equal(mean, o32.t[1]) and torch.equal(rstd, o32.t[2])
        else:
            LN.within("y", c, LN.row_err(y, y64), LN.row_err(c.y32 * fac, y64))
        LN.within("mean", c, LN.vec_err(mean, c.mean64, c.xmax), LN.vec_err(c.mean32, c.mean64, c.xmax))
        LN.within("rstd", c, LN.vec_err(rstd, c.rstd64, c.rstd64), LN.vec_err(c.rstd32, c.rstd64, c.rstd64))
    return rc, o, check


def ln_bwd(M, C, entry, add=False, p=0.0, flags=0, dz=True, dx_bf16=0):
    c, (L, s) = ln_case(M, C), lib()
    d, o = c.s, Outs()
    nblk = L.fs2hip_layernorm_bwd_blocks(M)
    dyb, zb = entry == "bwd_x" and bool(flags & 1), entry == "bwd_x" and bool(flags & 2)
    has_dz = entry == "bwd_dz" or (entry == "bwd_x" and dz)
    dyv = c.dy.bfloat16().float() if dyb else c.dy  # the values the kernel reads
    dx = o.new(M, C, dtype=bf16 if dx_bf16 else f32)
    part = o.new(nblk, 3 if has_dz else 2, C)
    dzt = o.new(M, C, dtype=bf16 if zb else f32) if has_dz else None
    dg = db = None
    common = (P(d["dy_b" if dyb else "dy"]), P(d["x"]), P(d["gamma"]), P(d["mean"]), P(d["rstd"]))
    addp = P(d["add"]) if add else None
    if entry == "bwd":
        dg, db = o.new(C), o.new(C)
        rc = L.fs2hip_layernorm_bwd(*common, addp, P(dx), P(part), P(dg), P(db), M, C, s)
    elif entry == "bwd_dz":
        rc = L.fs2hip_layernorm_bwd_dz(*common, addp, P(dx), P(dzt), DZ_SCALE, p, SEED, P(step()), P(part), M, C, s)
    elif entry == "bwd_x":
        rc = L.fs2hip_layernorm_bwd_x(*common, addp, P(dx), P(dzt), DZ_SCALE, p, SEED, P(step()), P(part), M, C, flags, s)
    else:
        rc = L.fs2hip_layernorm_bwd_pred(*common, P(dx), dx_bf16, P(part), M, C, p, SEED, P(step()), s)

    def check():
        fac = factors(p, M, C)
        mean_d, rstd_d = c.mean32.double(), c.rstd32.double()
        psum = part.sum(0, dtype=f64)
        if entry == "bwd_pred":  # test_backward_predictor_fp32 / test_bf16_predictor
            dym, pos = fac * c.dy, c.x > 0
            yard_x, yard_g, yard_b, dx32 = ln_yard(c, f"pred{p}", dym)
            full_exact = R.ln_bwd64(dym, c.x, c.gamma, c.mean64, c.rstd64)[0]
            full64 = R.ln_bwd64(dym, c.x, c.gamma, mean_d, rstd_d)[0]
            exact, dx64 = full_exact * pos, full64 * pos
            few = pos.sum(-1) < 2
            den = torch.where(few, full64.abs().amax(-1), dx64.abs().amax(-1))
            den_exact = torch.where(few, full_exact.abs().amax(-1), exact.abs().amax(-1))
            if dx_bf16:
                _, o32, _ = ln_bwd(M, C, "bwd_pred", p=p)
                assert torch.equal(dx, o32.t[0].bfloat16()) and torch.equal(part, o32.t[1])
            else:
                LN.within("pred dx", c, LN.row_err(dx, dx64, den), LN.row_err(dx32 * pos, exact, den_exact))
                assert bool((dx.cpu()[~pos] == 0).all())
            LN.check_param_sums(c, "pred", psum[0], psum[1], dym, mean_d, rstd_d, yard_g, yard_b)
            return
        yard_x, yard_g, yard_b, dx32 = ln_yard(c, "dyb" if dyb else "dy", dyv)
        dx64 = R.ln_bwd64(dyv, c.x, c.gamma, mean_d, rstd_d)[0]
        if add:
            exact = R.ln_bwd64(dyv, c.x, c.gamma, c.mean64, c.rstd64)[0] + c.add.double()
            dx64, yard_x = dx64 + c.add.double(), LN.row_err(dx32 + c.add, exact)
        LN.within("dx", c, LN.row_err(dx, dx64), yard_x)
        if entry == "bwd":
            LN.check_param_sums(c, "bwd", dg, db, dyv, mean_d, rstd_d, yard_g, yard_b)
        LN.check_param_sums(c, "partial", psum[0], psum[1], dyv, mean_d, rstd_d, yard_g, yard_b)
        if has_dz:  # test_backward_second_output_fp32 / test_bf16_second_output
            want = (dx.cpu() * torch.tensor(DZ_SCALE, dtype=f32)) * fac  # the kernel's products in the kernel's order
            assert torch.equal(dzt.cpu(), want.bfloat16() if zb else want)
            z = dzt.float().cpu()
            z64, zs = z.double().sum(0), z.double().abs().sum(0)
            LN.within("colsum(dz)", c, LN.vec_err(psum[2], z64, zs), LN.vec_err(z.sum(0), z64, zs))
    return rc, o, check


def ln_group(M, C):
    go = functools.partial
    yield "fwd", go(ln_fwd, M, C, "fwd")
    yield "fwd_b", go(ln_fwd, M, C, "fwd_b")
    for p in (0.0, 0.3):
        yield f"fwd_drop_p{p}", go(ln_fwd, M, C, "fwd_drop", p)
        for dxb in (0, 1):
            yield f"bwd_pred_xb{dxb}_p{p}", go(ln_bwd, M, C, "bwd_pred", p=p, dx_bf16=dxb)
    for add in (False, True):
        yield f"bwd_add{int(add)}", go(ln_bwd, M, C, "bwd", add=add)
        for p in (0.0, 0.3):
            yield f"bwd_dz_add{int(add)}_p{p}", go(ln_bwd, M, C, "bwd_dz", add=add, p=p)
    for flags in range(4):
        for dz in (False, True):
            yield f"bwd_x_f{flags}_dz{int(dz)}", go(ln_bwd, M, C, "bwd_x", add=True, p=0.3, flags=flags, dz=dz)


# ---------------------------------------------------------------------------------------------------------------------
# BatchNorm + activation and the column statistics (bn.hip)
# ---------------------------------------------------------------------------------------------------------------------
BN_EPS = 1e-5


@cached
def bn_case(M, C):
    g = torch.Generator().manual_seed(1000 * M + C)
    c = dict(M=M, C=C)
    c["y"] = torch.randn(M, C, generator=g) * 2 + 0.5
    c["dout"] = torch.randn(M, C, generator=g)
    c["gamma"], c["beta"] = 1 + 0.1 * torch.randn(C, generator=g), torch.randn(C, generator=g)
    c["rm"], c["rv"] = 0.1 * torch.randn(C, generator=g), torch.rand(C, generator=g) + 0.5
    for k in ("y", "dout"):
        c[k + "_d"], c[k + "_bd"] = dev(c[k]), dev(c[k].bfloat16())
    return c


def bn_values(c, k, as_bf16):
    return (c[k].bfloat16().float() if as_bf16 else c[k]).double()


@cached
def bn_stats(M, C, y_bf16, training):
    """[5, C] = (scale, shift, mean, invstd, eps) as fs2hip_bn_finalize writes them, from float64 statistics of the
    values the kernel reads; with the exact (mean, invstd) beside it"""
    c = bn_case(M, C)
    yv = bn_values(c, "y", y_bf16)
    mean, var = (yv.mean(0), yv.var(0, unbiased=False)) if training else (c["rm"].double(), c["rv"].double())
    inv = (var + BN_EPS) ** -0.5
    scale = c["gamma"].double() * inv
    st = torch.stack([scale, c["beta"].double() - mean * scale, mean, inv, torch.full_like(mean, BN_EPS)]).float()
    return dev(st), st.double(), mean, inv


ACTS = {0: (lambda t: t, lambda t: torch.ones_like(t)), 1: (torch.relu, lambda t: (t > 0).double())}


def bn_pre(st64, yv, act):
    pre = st64[0] * yv + st64[1]
    if act == 1:  # relu' jumps at 0: the fixed inputs keep every pre-activation clear of it (test_kernels_gpu.py's measure)
        assert bool((pre.abs() > 1e-5 * max(1.0, float(pre.abs().max()))).all()), "a pre-activation within rounding of 0"
    return pre


def colstats(M, C, in_bf16):
    c, (L, s) = bn_case(M, C), lib()
    o = Outs()
    nparts, rows = L.fs2hip_colstats_parts(M), L.fs2hip_colstats_part_rows(M)
    part = o.new(nparts, 2, C)
    rc = L.fs2hip_colstats_b(P(c["y_bd" if in_bf16 else "y_d"]), M, C, P(part), in_bf16, s)

    def check():
        yv = bn_values(c, "y", in_bf16)
        stripes = [yv[r0:r0 + rows] for r0 in range(0, M, rows)]
        close(part[:, 0], torch.stack([sp.mean(0) for sp in stripes]), 1e-5, "stripe means")
        close(part[:, 1], torch.stack([((sp - sp.mean(0)) ** 2).sum(0) for sp in stripes]), 1e-5, "stripe M2")
    return rc, o, check


def bn_fwd(M, C, in_bf16, which, act, p):
    c, (L, s) = bn_case(M, C), lib()
    o = Outs()
    st, st64, _, _ = bn_stats(M, C, bool(in_bf16), True)
    out = o.new(M, C) if which & 1 else None
    out_b = o.new(M, C, dtype=bf16) if which & 2 else None
    rc = L.fs2hip_bn_act_fwd_b(P(c["y_bd" if in_bf16 else "y_d"]), P(st), P(out), P(out_b), M, C, act, p, SEED,
                               P(step()), in_bf16, s)

    def check():
        ref = ACTS[act][0](bn_pre(st64, bn_values(c, "y", in_bf16), act)) * factors(p, M, C).double()
        if out is not None:
            near(out, ref, 2e-5, "bn fwd", floor_one=p > 0)
        if out is not None and out_b is not None:
            assert torch.equal(out_b, out.bfloat16())
        elif out_b is not None:
            near(out_b, ref, 2e-5, "bn fwd bf16", floor_one=p > 0, rounded=True)
    return rc, o, check


def bn_bwd(M, C, in_bf16, which, training, act, p):
    c, (L, s) = bn_case(M, C), lib()
    o = Outs()
    yb, dob = bool(in_bf16 & 1), bool(in_bf16 & 2)
    st, st64, mean, inv = bn_stats(M, C, yb, bool(training))
    nparts = max(L.fs2hip_colstats_parts(M), 1)
    part, coef = o.new(nparts, 2, C, scratch=True), o.new(2, C, scratch=True)
    dg, db = o.new(C), o.new(C)
    dy = o.new(M, C) if which & 1 else None
    dy_b = o.new(M, C, dtype=bf16) if which & 2 else None
    rc = L.fs2hip_bn_act_bwd_b(P(c["dout_bd" if dob else "dout_d"]), P(c["y_bd" if yb else "y_d"]), P(st), P(part),
                               P(coef), P(dg), P(db), P(dy), P(dy_b), M, C, act, p, SEED, P(step()), training, in_bf16, s)

    def check():
        yv = bn_values(c, "y", yb)
        dz = bn_values(c, "dout", dob) * factors(p, M, C).double() * ACTS[act][1](bn_pre(st64, yv, act))
        xhat = (yv - mean) * inv
        ref = st64[0] * (dz - dz.mean(0) - xhat * (dz * xhat).mean(0)) if training else st64[0] * dz
        # test_kernels_gpu.py: dy 5e-5, dgamma / dbeta 1e-4; test_dropout_gpu.py with dropout: 1e-4 of max(1, scale)
        tol = 1e-4 if p > 0 else 5e-5
        near(dg, (dz * xhat).sum(0), 1e-4, "bn dgamma", floor_one=p > 0)
        near(db, dz.sum(0), 1e-4, "bn dbeta", floor_one=p > 0)
        if dy is not None:
            near(dy, ref, tol, "bn dy", floor_one=p > 0)
        if dy is not None and dy_b is not None:
            assert torch.equal(dy_b, dy.bfloat16())
        elif dy_b is not None:
            near(dy_b, ref, tol, "bn dy bf16", floor_one=p > 0, rounded=True)
    return rc, o, check


def bn_group(kind):
    go = functools.partial
    if kind == "colstats":
        for M, C in ((16, 64), (17, 64), (17, 1028)):
            for ib in (0, 1):
                yield f"M{M}_C{C}_in{ib}", go(colstats, M, C, ib)
    elif kind == "fwd":
        for ib in (0, 1):
            for which in range(4):
                for act in (0, 1):
                    for p in (0.0, 0.3):
                        yield f"in{ib}_out{which}_act{act}_p{p}", go(bn_fwd, 17, 64, ib, which, act, p)
        yield "C1028", go(bn_fwd, 17, 1028, 0, 1, 0, 0.0)
    else:
        M = int(kind[len("bwd_m"):])
        for ib in range(4):
            for which in range(4):
                for tr in (0, 1):
                    for act in (0, 1):
                        for p in (0.0, 0.3):
                            yield f"in{ib}_out{which}_train{tr}_act{act}_p{p}", go(bn_bwd, M, 64, ib, which, tr, act, p)
        yield "C1028", go(bn_bwd, M, 1028, 0, 1, 1, 0, 0.0)


# ---------------------------------------------------------------------------------------------------------------------
# depthwise convolution (conv.hip)
# ---------------------------------------------------------------------------------------------------------------------
DW_B, DW_T = 2, 70  # two time blocks of 64 steps, the second partial
DW_KS = (3, 5, 7, 9, 15, 31, 11, 63, 4, 65)


@cached
def dw_case(C, K):
    g = torch.Generator().manual_seed(100 * K + C)
    c = dict(x2=torch.randn(DW_B * DW_T, 2 * C, generator=g), x1=torch.randn(DW_B * DW_T, C, generator=g),
             w=0.3 * torch.randn(K, C, generator=g), bias=0.1 * torch.randn(C, generator=g),
             dy=torch.randn(DW_B, DW_T, C, generator=g))
    for k in ("x2", "x1", "dy"):
        c[k + "_d"], c[k + "_bd"] = dev(c[k]), dev(c[k].bfloat16())
    c["w_d"], c["bias_d"] = dev(c["w"]), dev(c["bias"])
    return c


@cached
def dw_ref(C, K, glu, in_bf16):
    """float64 F.conv1d, forward and backward, on the values the kernel reads: (y, dx, dw [K, C], dbias)"""
    c = dw_case(C, K)
    rd = (lambda t: t.bfloat16().float().double()) if in_bf16 else (lambda t: t.double())
    x = rd(c["x2" if glu else "x1"]).view(DW_B, DW_T, -1).requires_grad_(True)
    w = c["w"].double().t().contiguous()[:, None, :].requires_grad_(True)
    b = c["bias"].double().requires_grad_(True)
    a = F.glu(x, dim=-1) if glu else x
    y = F.conv1d(a.transpose(1, 2), w, b, padding=(K - 1) // 2, groups=C).transpose(1, 2)
    y.backward(rd(c["dy"]))
    return y.detach(), x.grad.reshape(DW_B * DW_T, -1), w.grad[:, 0, :].t(), b.grad


class env:
    """environment variables the library reads at every call, for the length of one launch"""

    def __init__(self, pairs):
        self.pairs, self.saved = dict(pairs or ()), {}

    def __enter__(self):
        for k, v in self.pairs.items():
            self.saved[k] = os.environ.get(k)
            os.environ[k] = v

    def __exit__(self, *exc):
        for k, v in self.saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        return False


def dw_fwd(C, K, glu, stats, io, envs=None):
    c, (L, s) = dw_case(C, K), lib()
    o = Outs()
    x = c[("x2" if glu else "x1") + ("_bd" if io == 1 else "_d")]
    y = o.new(DW_B, DW_T, C, dtype=bf16 if io else f32)
    nparts = L.fs2hip_dwconv_blocks(DW_B, DW_T)
    part = o.new(nparts, 2, C) if stats else None
    with env(envs):
        rc = L.fs2hip_dwconv_fwd_b(P(x), x.shape[-1], P(c["w_d"]), P(c["bias_d"]), P(y), P(part), DW_B, DW_T, C, K, glu,
                                   stats, io, s)

    def check():
        ref = dw_ref(C, K, glu, io == 1)[0]
        near(y, ref, 2e-5, "dwconv fwd", rounded=bool(io))
        if stats:  # of the values as written (a bf16 y: of the rounded ones), per stripe of 64 steps
            seen = y.float().cpu().double() if io else ref
            stripes = [seen[bb, t0:t0 + 64] for bb in range(DW_B) for t0 in range(0, DW_T, 64)]
            assert nparts == len(stripes)
            close(part[:, 0], torch.stack([sp.mean(0) for sp in stripes]), 1e-5, "stripe means")
            close(part[:, 1], torch.stack([((sp - sp.mean(0)) ** 2).sum(0) for sp in stripes]), 1e-5, "stripe M2")
    return rc, o, check


def dw_bwd(C, K, glu, dxb, with_dw, envs=None):
    c, (L, s) = dw_case(C, K), lib()
    o = Outs()
    sfx = "_bd" if dxb & 2 else "_d"
    x, dy = c[("x2" if glu else "x1") + sfx], c["dy" + sfx]
    dx = o.new(*x.shape, dtype=bf16 if dxb & 1 else f32)
    nblk = L.fs2hip_dwconv_blocks(DW_B, DW_T)
    part = o.new(nblk, K + 1, C, scratch=with_dw)
    dw, db = (o.new(K, C), o.new(C)) if with_dw else (None, None)
    with env(envs):
        rc = L.fs2hip_dwconv_bwd_b(P(dy), P(x), x.shape[-1], P(c["w_d"]), P(dx), dxb, P(part), P(dw), P(db), DW_B, DW_T,
                                   C, K, glu, s)

    def check():
        _, dx_ref, dw_ref_, db_ref = dw_ref(C, K, glu, bool(dxb & 2))
        near(dx, dx_ref, 2e-5, "dwconv dx", rounded=bool(dxb & 1))
        if with_dw:
            close(dw, dw_ref_, 1e-4, "dwconv dw")
            close(db, db_ref, 1e-4, "dwconv db")
        else:  # the partial sums the caller finishes: [block][K taps | bias][C]
            psum = part.sum(0, dtype=f64)
            close(psum[:K], dw_ref_, 1e-4, "dwconv dw partial sums")
            close(psum[K], db_ref, 1e-4, "dwconv db partial sums")
    return rc, o, check


def dw_fwd_forms(C, K, tag="", envs=None):
    for glu in (0, 1):
        for stats in (0, 1):
            for io in (0, 1, 2):
                yield f"fwd{tag}_C{C}_K{K}_glu{glu}_stats{stats}_io{io}", functools.partial(dw_fwd, C, K, glu, stats, io, envs)


def dw_bwd_forms(C, K, tag="", envs=None):
    for glu in (0, 1):
        for dxb in range(4):
            for with_dw in (0, 1):
                yield f"bwd{tag}_C{C}_K{K}_glu{glu}_dxb{dxb}_dw{with_dw}", functools.partial(dw_bwd, C, K, glu, dxb, with_dw, envs)


def dw_group(kind, C):
    if kind == "env":
        for tag, envs in (("_tile0", (("FS2_DWCONV_TILE", "0"),)), ("_generic1", (("FS2_DWCONV_GENERIC", "1"),))):
            for K in (7, 11):
                yield from dw_fwd_forms(C, K, tag, envs)
                yield from dw_bwd_forms(C, K, tag, envs)
    else:
        for K in DW_KS:
            yield from (dw_fwd_forms if kind == "fwd" else dw_bwd_forms)(C, K)


# ---------------------------------------------------------------------------------------------------------------------
# attention (attention.hip, attention2.hip, attention_bf16.hip)
# ---------------------------------------------------------------------------------------------------------------------
AT_B, AT_T, AT_H, AT_LENS = 2, 70, 2, (70, 37)
AT_HDS = (16, 32, 64, 128, 256, 24, 0, 257)
ATB_T, ATB_LENS = 130, (130, 37)


def attn_ref64(qkv, dout, lens, B, T, Hh, hd, fac):
    """softmax(Q K^T / sqrt(hd) + key-padding mask) (* dropout factors) V per head in float64, the log-sum-exp of each
    query row, and the gradient of sum(o * dout): test_attention_gpu.py's reference with the kernels' own mask"""
    qr = qkv.double().view(B, T, -1).requires_grad_(True)
    q, k, v = qr.view(B, T, 3, Hh, hd).permute(2, 0, 3, 1, 4)
    sc = (q @ k.transpose(-1, -2)) / math.sqrt(hd)
    pad = torch.arange(T)[None, :] >= torch.tensor(lens)[:, None]
    sc = sc.masked_fill(pad[:, None, None, :], float("-inf"))
    pr = torch.softmax(sc, dim=-1)
    if fac is not None:
        pr = pr * fac.double()
    o = (pr @ v).permute(0, 2, 1, 3).reshape(B, T, Hh * hd)
    o.backward(dout.double().view(B, T, -1))
    return o.detach(), torch.logsumexp(sc, dim=-1).detach(), qr.grad


def pad_heads(x, groups, hd, hdp):
    """[rows][groups * hd] -> [rows][groups * hdp], zero pad columns"""
    return F.pad(x.reshape(-1, groups, hd), (0, hdp - hd)).reshape(-1, groups * hdp)


def cut_heads(x, groups, hd, hdp):
    return x.reshape(-1, groups, hdp)[..., :hd].reshape(-1, groups * hd)


def attn_mask(p, B, T, Hh):
    """the probabilities' dropout factors: element index in [B, H, T, T rounded up to even] (tests/dropout_masks.py)"""
    if not p > 0:
        return None
    Tp = T + (T & 1)
    return R.drop_factors(p, SEED, None, B * Hh * T * Tp).view(B, Hh, T, Tp)[..., :T]


@cached
def attn_case(HD):
    """inputs at head dimension HD, laid out at the width the kernels run it at (zero pad columns)"""
    B, T, Hh = AT_B, AT_T, AT_H
    g = torch.Generator().manual_seed(7 * HD + T)
    HDk = H.attention_padded_dim(HD)
    qkv, dout = torch.randn(B * T, 3 * Hh * HD, generator=g), torch.randn(B * T, Hh * HD, generator=g)
    c = dict(HD=HD, HDk=HDk, qkv=qkv, dout=dout)
    c["qkv_d"], c["dout_d"] = dev(pad_heads(qkv, 3 * Hh, HD, HDk)), dev(pad_heads(dout, Hh, HD, HDk))
    c["lens_d"] = torch.tensor(AT_LENS, dtype=torch.int32, device="cuda")
    return c


@cached
def attn_refs(HD, p, rounded):
    """(o, lse, dqkv) in float64; ``rounded``: on bf16-rounded q, k, v, dout (the bf16-operand kernels' reference)"""
    c = attn_case(HD)
    rd = (lambda t: t.bfloat16().float()) if rounded else (lambda t: t)
    return attn_ref64(rd(c["qkv"]), rd(c["dout"]), AT_LENS, AT_B, AT_T, AT_H, HD, attn_mask(p, AT_B, AT_T, AT_H))


def attn_tols(op):
    """(o, lse, dqkv): test_attention_gpu.py -- fp32 and "32-split" 2e-5 / 2e-5 of max(1, scale) and 3e-5 of the
    gradient's scale; bf16 operands 1e-2 / 1e-2 / 2e-2 against the reference on rounded operands"""
    return (1e-2, 1e-2, 2e-2) if op == 1 else (2e-5, 2e-5, 3e-5)


def attn_fwd(HD, op, p, keep):
    c, (L, s) = attn_case(HD if 0 < HD <= 256 else 16), lib()
    B, T, Hh, o = AT_B, AT_T, AT_H, Outs()
    out, lse = o.new(B * T, Hh * c["HDk"]), o.new(B, Hh, T)
    sc = o.new(B, Hh, T, (T + 31) // 32 * 32) if keep else None
    rc = L.fs2hip_attention_fwd(P(c["qkv_d"]), P(c["lens_d"]), P(out), P(lse), P(sc), sc.numel() if keep else 0, B, T, Hh,
                                HD, p, SEED, None, op, s)
    o.scores = sc

    def check():
        ro, rl, _ = attn_refs(HD, p, op == 1)
        to, tl, _ = attn_tols(op)
        near(cut_heads(out, Hh, HD, c["HDk"]), ro.reshape(B * T, -1), to, "attention o", floor_one=True)
        near(lse, rl, tl, "attention lse", floor_one=True)
        if c["HDk"] != HD:  # the pad columns of o are exact zeros
            assert float(out.view(B * T, Hh, -1)[..., HD:].abs().max()) == 0.0
    return rc, o, check


def attn_bwd(HD, op, p, spill, kept):
    c, (L, s) = attn_case(HD if 0 < HD <= 256 else 16), lib()
    B, T, Hh, o = AT_B, AT_T, AT_H, Outs()
    hd, HDk = c["HD"], c["HDk"]
    ro, rl, rg = attn_refs(hd, p, op == 1)
    key = ("attn_bwd_in", hd, p, op == 1)
    if key not in _CACHE:  # o and lse as the forward pass leaves them: the reference's, in fp32
        _CACHE[key] = dev(pad_heads(ro.float().reshape(B * T, -1), Hh, hd, HDk)), dev(rl.float())
    o_d, lse_d = _CACHE[key]
    n = B * Hh * T * ((T + 31) // 32 * 32)
    scores = None
    if kept:  # what the forward pass kept, where it keeps any; otherwise a buffer of the right size
        rc_f, of, _ = attn_fwd(HD, op, p, True)
        scores = of.scores if rc_f == 0 else torch.zeros(n, device="cuda")
    dqkv = o.new(B * T, 3 * Hh * HDk)
    aux = o.new(2 * B * Hh * T + 4, scratch=True)
    ds = o.new(n, scratch=True) if spill else None
    rc = L.fs2hip_attention_bwd(P(c["qkv_d"]), P(c["lens_d"]), P(o_d), P(c["dout_d"]), P(lse_d), P(scores), P(aux), P(ds),
                                n if spill else 0, P(dqkv), B, T, Hh, HD, p, SEED, None, op, s)

    def check():
        near(cut_heads(dqkv, 3 * Hh, hd, HDk), rg.reshape(B * T, -1), attn_tols(op)[2], "attention dqkv")
    return rc, o, check


@cached
def attnb_case(HD):
    B, T, Hh = AT_B, ATB_T, AT_H
    g = torch.Generator().manual_seed(B * 1000 + T + HD)
    c = dict(qkv=torch.randn(B * T, 3 * Hh * HD, generator=g).bfloat16(),
             dout=torch.randn(B * T, Hh * HD, generator=g).bfloat16())
    c["qkv_d"], c["dout_d"] = dev(c["qkv"]), dev(c["dout"])
    c["lens_d"] = torch.tensor(ATB_LENS, dtype=torch.int32, device="cuda")
    return c


@cached
def attnb_refs(HD, p):
    c = attnb_case(HD)
    return attn_ref64(c["qkv"].float(), c["dout"].float(), ATB_LENS, AT_B, ATB_T, AT_H, HD, attn_mask(p, AT_B, ATB_T, AT_H))


def rel_l2(a, b):
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def attnb_fwd(HD, p):
    c, (L, s) = attnb_case(HD), lib()
    B, T, Hh, o = AT_B, ATB_T, AT_H, Outs()
    out, lse = o.new(B * T, Hh * HD, dtype=bf16), o.new(B, Hh, T)
    rc = L.fs2hip_attention_fwd_b(P(c["qkv_d"]), P(c["lens_d"]), P(out), P(lse), B, T, Hh, HD, p, SEED, None, s)

    def check():  # test_attention_bf16_storage_gpu.py: relative L2 1e-2, largest element 3e-2 of the scale, lse 2e-3
        ro, rl, _ = attnb_refs(HD, p)
        got, ro = out.float().cpu().double(), ro.reshape(B * T, -1)
        assert bool(torch.isfinite(got).all()) and rel_l2(got, ro) < 1e-2
        assert float((got - ro).abs().max()) < 3e-2 * float(ro.abs().max())
        near(lse, rl, 2e-3, "attention_b lse", floor_one=True)
    return rc, o, check


def attnb_bwd(HD, p, spill):
    c, (L, s) = attnb_case(HD), lib()
    B, T, Hh, o = AT_B, ATB_T, AT_H, Outs()
    D = Hh * HD
    ro, rl, rg = attnb_refs(HD, p)
    key = ("attnb_bwd_in", HD, p)
    if key not in _CACHE:
        _CACHE[key] = dev(ro.reshape(B * T, -1).bfloat16()), dev(rl.float())
    o_d, lse_d = _CACHE[key]
    n = B * Hh * T * ((T + 31) // 32 * 32)
    dqkv = o.new(B * T, 3 * D, dtype=bf16)
    aux = o.new(2 * B * Hh * T + 4, scratch=True)
    ds = o.new(n, dtype=bf16, scratch=True) if spill else None
    rc = L.fs2hip_attention_bwd_b(P(c["qkv_d"]), P(c["lens_d"]), P(o_d), P(c["dout_d"]), P(lse_d), P(aux), P(ds),
                                  n if spill else 0, P(dqkv), B, T, Hh, HD, p, SEED, None, s)

    def check():  # per part against the whole gradient's scale: relative L2 1.5e-2, largest element 3e-2
        got, gref = dqkv.float().cpu().double(), rg.reshape(B * T, -1)
        assert bool(torch.isfinite(got).all())
        gmax, gnorm = float(gref.abs().max()), float(gref.norm())
        for nm, sl in (("dq", slice(0, D)), ("dk", slice(D, 2 * D)), ("dv", slice(2 * D, 3 * D))):
            d = got[..., sl] - gref[..., sl]
            e2 = float(d.norm()) / max(float(gref[..., sl].norm()), 1e-2 * gnorm)
            em = float(d.abs().max()) / max(float(gref[..., sl].abs().max()), 1e-1 * gmax)
            print(f"attention_b {nm}: l2 {e2:.3e} max {em:.3e}")
            assert e2 < 1.5e-2 and em < 3e-2, (nm, e2, em)
    return rc, o, check


def attn_pad(unpad):
    (L, s), o = lib(), Outs()
    rows, groups, hd, hdp = 9, 6, 24, 32
    src = torch.randn(rows, groups * (hdp if unpad else hd), generator=torch.Generator().manual_seed(3))
    src_d = dev(src)
    dst = o.new(rows, groups * (hd if unpad else hdp))
    if unpad:
        rc = L.fs2hip_attention_unpad_heads(P(src_d), P(dst), rows, groups, hdp, hd, s)
    else:
        rc = L.fs2hip_attention_pad_heads(P(src_d), P(dst), rows, groups, hd, hdp, s)

    def check():
        assert torch.equal(dst.cpu(), cut_heads(src, groups, hd, hdp) if unpad else pad_heads(src, groups, hd, hdp))
    return rc, o, check


def attn_group(kind):
    go = functools.partial
    if kind == "fwd":
        for HD in AT_HDS:
            for op in range(4):
                for p in (0.0, 0.2):
                    for keep in (0, 1):
                        yield f"HD{HD}_op{op}_p{p}_scores{keep}", go(attn_fwd, HD, op, p, keep)
    elif kind == "bwd":
        for HD in AT_HDS:
            for op in range(4):
                for p in (0.0, 0.2):
                    for spill, kept in ((0, 0), (1, 0), (1, 1), (0, 1)):
                        yield f"HD{HD}_op{op}_p{p}_ds{spill}_scores{kept}", go(attn_bwd, HD, op, p, spill, kept)
    elif kind == "b":
        for HD in (128, 64):
            for p in (0.0, 0.2):
                yield f"fwd_b_HD{HD}_p{p}", go(attnb_fwd, HD, p)
                for spill in (0, 1):
                    yield f"bwd_b_HD{HD}_p{p}_ds{spill}", go(attnb_bwd, HD, p, spill)
    elif kind == "pad":
        yield "pad_heads", go(attn_pad, False)
        yield "unpad_heads", go(attn_pad, True)
    else:  # the first-generation kernels at the head dims the second generation has taken over: FS2_ATTN_GEN1 set
        assert os.environ.get("FS2_ATTN_GEN1"), "this group runs in a process started with FS2_ATTN_GEN1"
        for HD in (64, 128):
            for op in (0, 1):
                yield f"fwd_HD{HD}_op{op}", go(attn_fwd, HD, op, 0.0, 0)
                yield f"bwd_HD{HD}_op{op}", go(attn_bwd, HD, op, 0.0, 0, 0)


# ---------------------------------------------------------------------------------------------------------------------
# the groups, their verification and their recording
# ---------------------------------------------------------------------------------------------------------------------
GROUPS = {f"layernorm_M{M}_C{C}": functools.partial(ln_group, M, C) for M, C in LN_SHAPES}
GROUPS.update({f"batchnorm_{k}": functools.partial(bn_group, k) for k in ("colstats", "fwd", "bwd_m16", "bwd_m17")})
GROUPS.update({f"dwconv_{k}_C{C}": functools.partial(dw_group, k, C) for k in ("fwd", "bwd", "env") for C in (64, 40)})
GROUPS.update({f"attention_{k}": functools.partial(attn_group, k) for k in ("fwd", "bwd", "b", "pad")})
CHILD_GROUP = "attention_gen1"


def run_group(name):
    """{case: [return code, digest or None]} of one group, every launch checked against its float64 reference"""
    got, failed = {}, []
    for case, go in (attn_group("gen1") if name == CHILD_GROUP else GROUPS[name]()):
        rc, outs, check = go()
        torch.cuda.synchronize()
        try:
            assert outs.slack_untouched(), f"{name} {case}: wrote outside its tensors"
            if rc == 0:
                check()
            else:
                assert outs.untouched(), f"{name} {case}: refused with {rc} after writing to an output"
        except AssertionError as e:
            failed.append(f"{name} {case}: {e}")
        got[case] = [rc, outs.digest() if rc == 0 else None]
    _CACHE.clear()
    return got, failed


def run_child():
    """the FS2_ATTN_GEN1 group in a fresh process of its own: (results, failures)"""
    r = subprocess.run([sys.executable, str(Path(__file__).resolve()), "--child"], timeout=300, capture_output=True,
                       text=True, env={**os.environ, "FS2_ATTN_GEN1": "1"})
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    assert r.returncode == 0 and len(lines) == 1, f"child exited with {r.returncode}:\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}"
    return json.loads(lines[0][len("RESULT "):])


def compare(name, got, failed):
    want = json.loads(GOLDEN.read_text())[name]
    assert sorted(got) == sorted(want), f"{name}: the cases differ from the recorded ones"
    for case, (rc, dg) in got.items():
        rc_want, dg_want = want[case]
        assert rc == rc_want, f"{name} {case}: return code {rc}, recorded {rc_want}"
        if dg_want is not None:
            assert dg == dg_want, f"{name} {case}: output bytes differ from the recorded launch"
    assert not failed, "\n".join(failed)


@pytest.mark.parametrize("name", list(GROUPS))
def test_launches_accept_refuse_and_compute_as_recorded(name):
    compare(name, *run_group(name))


def test_first_generation_attention_at_64_and_128_as_recorded():
    compare(CHILD_GROUP, *run_child())


def record(path):
    passes, failed = [], []
    for _ in range(2):
        got = {}
        for name in GROUPS:
            got[name], bad = run_group(name)
            failed += bad
        got[CHILD_GROUP], bad = run_child()
        failed += bad
        passes.append(got)
    first, second = passes
    dropped = 0
    for name, cases in first.items():
        for case, (rc, dg) in cases.items():
            assert second[name][case][0] == rc, (name, case)
            if second[name][case][1] != dg:
                print(f"NOT REPRODUCED: {name} {case}: {dg} then {second[name][case][1]}; digest dropped")
                cases[case][1] = None
                dropped += 1
    Path(path).parent.mkdir(parents=True, exist_ok=True)
    Path(path).write_text(json.dumps(first, separators=(",", ":"), sort_keys=True).replace("},", "},\n") + "\n")
    n = sum(len(v) for v in first.values())
    ok = sum(1 for v in first.values() for rc, _ in v.values() if rc == 0)
    print(f"recorded {n} launches ({ok} accepted, {dropped} digests dropped) in {len(first)} groups -> {path}")
    assert not failed, "accepted launches off their float64 reference (do not commit this recording):\n" + "\n".join(failed)


if __name__ == "__main__":
    if sys.argv[1:2] == ["--child"]:
        print("RESULT " + json.dumps(run_group(CHILD_GROUP)))
    else:
        assert sys.argv[1:2] == ["--record"], "usage: python tests/test_launch_dispatch_gpu.py --record [path]"
        record(sys.argv[2] if len(sys.argv) > 2 else GOLDEN)
