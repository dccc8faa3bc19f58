"""Which launches ``fs2hip_gemm`` / ``fs2hip_gemm_grouped`` accept and what they compute, tile id by tile id, at the
smallest shapes that take each branch of the host-side launch code (csrc/gemm_launch.h, csrc/gemm_tiles.h): every
operand orientation and operand mode, the conv-tap modes on both sides of each core's K-tile, split-K with and without
empty slices, the weights-stationary and split-tail forms, the fused epilogues, grouped launches.

Every case is launched with ``a.tile`` forced to every id the binding knows, to 0 and to ids no table has.  The return
code must be the recorded one; an accepted launch must match the float64 product under the tolerance the GEMM tests
use for its operand mode (test_kernels_gpu.py, test_gemm_bf16_gpu.py, test_gemm_split_gpu.py,
test_gemm_bf16_storage_gpu.py) AND reproduce the recorded SHA-256 prefix of its output bytes: the launch code may be
reorganised, the kernels, grids and arguments it ends in may not change.  Outputs are NaN before every launch, so an
element no kernel writes fails the comparison.

tests/golden/gemm_dispatch.json is recorded on the GPU from the commit BEFORE a change to the launch code:
``python tests/test_gemm_dispatch_gpu.py --record [path]`` (two passes; a digest that differs between them is dropped,
the return code and the float64 check stay)."""
import ctypes
import hashlib
import json
import math
import sys
from pathlib import Path

import pytest
import torch
import torch.nn.functional as F

REPO = Path(__file__).resolve().parent.parent
if __name__ == "__main__" and str(REPO) not in sys.path:
    sys.path.insert(0, str(REPO))

from fastspeech2_lightning_amd import hip as H  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = REPO / "tests" / "golden" / "gemm_dispatch.json"
IDS = sorted(set(H.GEMM_TILES) | set(H.GEMM_TILES_B) | {0, 16, 27, 34})
GROUP_IDS = sorted({t for v in H.GROUP_TILES.values() for t in v} | {0, 4})  # 4: a tile the grouped kernels lack
NT, NN, TN, TT = (1, 1), (1, 0), (0, 0), (0, 1)  # (a_kcontig, b_kcontig); TT: only the register-staged core takes it
ONAME = {NT: "nt", NN: "nn", TN: "tn", TT: "tt"}
#: the register-staged core has no bf16 instance: with operand_bf16 1 / 2 these tiles multiply in exact fp32 (include/fs2hip.h)
STAGED = (1, 2, 3)
PAD = 1 << 16  # elements of slack on both sides of every device tensor


def rnd(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def dev(t):
    buf = torch.zeros(t.numel() + 2 * PAD, dtype=t.dtype, device="cuda")
    v = buf[PAD:PAD + t.numel()].view(t.shape)
    v.copy_(t)
    return v


def out_buf(*shape):
    n = math.prod(shape)
    return torch.empty(n + 2 * PAD, device="cuda")[PAD:PAD + n].view(shape)


def case(name, orient, mode, Mc=200, Nc=80, R=128, taps=1, T=0, shift=0, splitk=1, colsum=False, epi=H.EPI_STORE,
         act=None, out_pre=False, drop=0.0, seed=0):
    return dict(name=name, orient=orient, mode=mode, Mc=Mc, Nc=Nc, R=R, taps=taps, T=T, shift=shift, splitk=splitk,
                colsum=colsum, epi=epi, act=act, out_pre=out_pre, drop=drop, seed=seed)


def _cases():
    cs = []
    for mode in (0, 4):
        for o in (NT, NN, TN, TT):
            cs.append(case(f"plain_{ONAME[o]}_m{mode}", o, mode))
    cs.append(case("plain_nt_m0_n64", NT, 0, Nc=64))
    for mode in (1, 2):
        for o in (NT, NN, TN):
            cs.append(case(f"plain_{ONAME[o]}_m{mode}", o, mode))
    cs.append(case("plain_nt_m3", NT, 3))
    # convolution over the rows of A (shift_operand = 0): Mc = 2 T rows, three taps of Rper columns
    for mode in (0, 4):
        for o in (NT, NN):
            cs.append(case(f"conv0_{ONAME[o]}_rper64_m{mode}", o, mode, R=192, taps=3, T=100))
        cs.append(case(f"conv0_nt_rper32_m{mode}", NT, mode, R=96, taps=3, T=100))
        cs.append(case(f"conv0_nt_rper16_m{mode}", NT, mode, R=48, taps=3, T=100))
    cs.append(case("conv0_nn_rper16_m0", NN, 0, R=48, taps=3, T=100))
    cs.append(case("conv0_nt_rper64_m3", NT, 3, R=192, taps=3, T=100))
    # convolution weight gradient (shift_operand = 1): two utterances of T rows in the reduction, one slice per tap
    for mode in (0, 4):
        for T in (64, 32, 16):
            cs.append(case(f"conv1_tn_t{T}_m{mode}", TN, mode, R=2 * T, taps=3, T=T, shift=1))
    for mode in (0, 4):
        cs.append(case(f"split2_tn_r256_m{mode}", TN, mode, R=256, splitk=2))
        cs.append(case(f"split4_tn_r64_m{mode}", TN, mode, R=64, splitk=4))  # chunks of one K-tile: empty slices
        cs.append(case(f"split2_tn_r256_colsum_m{mode}", TN, mode, R=256, splitk=2, colsum=True))
    # weights-stationary and split-tail forms
    for mode in (0, 4):
        cs.append(case(f"ws_nt_n256_r256_m{mode}", NT, mode, Nc=256, R=256))
    cs.append(case("ws_nt_n128_r1024_m4", NT, 4, Nc=128, R=1024))
    cs.append(case("ws_nt_n256_r256_resid_m4", NT, 4, Nc=256, R=256, epi=H.EPI_RESID))
    cs.append(case("ws_nt_n128_r1024_resid_m4", NT, 4, Nc=128, R=1024, epi=H.EPI_RESID))
    cs.append(case("ws_nt_n256_r256_silu_pre_m0", NT, 0, Nc=256, R=256, epi=H.EPI_ACT, act="silu", out_pre=True))
    cs.append(case("ws_nt_n256_r256_relu_drop_m4", NT, 4, Nc=256, R=256, epi=H.EPI_ACT, act="relu", drop=0.3))
    return cs


CASES = _cases()
# grouped launches: two members of one orientation and operand class, different shapes; the second weight gradient is split
GROUPS = [(f"group_{ONAME[o]}_m{mode}", o, mode) for mode in (0, 4) for o in (NT, NN, TN, TT)]


def quant(t, mode):
    """float64 values of what the kernel multiplies: modes 1 rounds fp32 operands to bf16 in registers, 3 / 4 read bf16"""
    return t.bfloat16().double() if mode in (1, 3, 4) else t.double()


def shift_rows(x, s, T):
    """row i of the result = row i + s of x inside the same utterance of T rows, else zero (conv 'same' padding)"""
    out = torch.zeros_like(x)
    t = torch.arange(x.shape[0]) % T + s
    ok = (t >= 0) & (t < T)
    idx = torch.arange(x.shape[0])[ok]
    out[idx] = x[idx + s]
    return out


class Built:
    """One launch's arguments, device tensors and float64 references."""

    def __init__(self, c):
        self.c = c
        mode, (akc, bkc) = c["mode"], c["orient"]
        Mc, Nc, R, taps, T, S = c["Mc"], c["Nc"], c["R"], c["taps"], c["T"], c["splitk"]
        store = (lambda t: t.bfloat16()) if mode >= 3 else (lambda t: t)
        sd = 10 * c["seed"]
        a = H.GemmArgs()
        a.Mc, a.Nc, a.R, a.a_kcontig, a.b_kcontig = Mc, Nc, R, akc, bkc
        a.taps, a.T, a.shift_operand, a.splitk, a.alpha, a.res_scale, a.operand_bf16 = taps, T, c["shift"], S, 1.0, 1.0, mode
        self.keep = []
        self.ref_fp32 = None  # modes 1 / 2 only: the exact product, which is what the register-staged core computes
        ntap_out = 1
        if c["shift"] == 1:  # A = dy [R][Mc], B = x [R][Nc]; slice j multiplies dy with x shifted by j - 1 rows
            dy, x = rnd(R, Mc, seed=sd + 1), rnd(R, Nc, seed=sd + 2, scale=R ** -0.5)
            Ad, Bd = dev(store(dy)), dev(store(x))
            a.lda, a.ldb, a.tap_mul, a.tap_add, a.c_tap_stride = Mc, Nc, 1, -1, Mc * Nc
            ref = torch.stack([quant(dy, mode).t() @ shift_rows(quant(x, mode), j - 1, T) for j in range(taps)])
            ntap_out = taps
            colref = quant(dy, mode).sum(0)
        else:
            Rper = R // taps
            x = rnd(Mc, Rper, seed=sd + 1)
            w = rnd(taps, Rper, Nc, seed=sd + 2, scale=R ** -0.5)  # [tap][k][n]
            Ad = dev(store(x if akc else x.t().contiguous()))
            Bd = dev(store(w.transpose(1, 2).contiguous() if bkc else w))
            a.lda, a.ldb, a.b_tap_stride = (Rper if akc else Mc), (Rper if bkc else Nc), Rper * Nc
            a.tap_mul, a.tap_add = (1, -((taps - 1) // 2)) if bkc else (-1, (taps - 1) // 2)
            xq, wq = quant(x, mode), quant(w, mode)
            if taps == 1:
                ref = xq @ wq[0]
                if mode in (1, 2):
                    self.ref_fp32 = (x.double() @ w[0].double())[None]
            else:
                ref = sum(shift_rows(xq, j * a.tap_mul + a.tap_add, T) @ wq[j] for j in range(taps))
            ref = ref[None]
            colref = xq.sum(1)
        a.A, a.B = Ad.data_ptr(), Bd.data_ptr()
        self.keep += [Ad, Bd]
        self.C = out_buf(ntap_out, Mc, Nc)
        a.C, a.ldc = self.C.data_ptr(), Nc
        self.ws = out_buf(8 * ntap_out * Mc * Nc)  # split-K slabs, or scratch of the split-tail tiles
        a.workspace, a.workspace_floats = self.ws.data_ptr(), self.ws.numel()
        self.outs = [self.C, self.ws]
        self.pre = self.colsum = None
        if S == 1 and (akc or bkc):
            bias = rnd(Nc, seed=sd + 3)
            bd = dev(bias)
            self.keep.append(bd)
            a.bias = bd.data_ptr()
            ref = ref + bias.double()
            if self.ref_fp32 is not None:
                self.ref_fp32 = self.ref_fp32 + bias.double()
        a.epi = c["epi"]
        a.act = H._ACT[c["act"]]
        self.checks = []  # (what, tensor getter, float64 reference)
        if c["epi"] == H.EPI_ACT:
            fn = {"silu": F.silu, "relu": torch.relu}[c["act"]]
            if c["out_pre"]:
                self.pre = out_buf(1, Mc, Nc)
                a.out_pre, a.ldpre = self.pre.data_ptr(), Nc
                self.outs.append(self.pre)
                self.checks.append(("pre-activation", lambda: self.pre, ref))
            ref = fn(ref)
            if c["drop"] > 0:
                step = torch.zeros(1, dtype=torch.int64, device="cuda")
                d = H.Drop(c["drop"], 0x1234567, step)
                a.drop_p, a.drop_seed, a.drop_step = d.p, d.seed, d.step_ptr
                factors = H.axpby(torch.ones(Mc * Nc, device="cuda"), None, 1.0, 0.0, d).view(1, Mc, Nc).cpu()
                keep = float((factors != 0).float().mean())
                assert abs(keep - (1 - c["drop"])) < 0.02, keep
                ref = ref * factors.double()
                self.keep.append(step)
        elif c["epi"] == H.EPI_RESID:
            r = rnd(Mc, Nc, seed=sd + 4)
            rd = dev(r)
            self.keep.append(rd)
            a.resid, a.ldr, a.res_scale = rd.data_ptr(), Nc, 0.5
            ref = r.double() + 0.5 * ref
        if c["colsum"]:
            self.colsum = out_buf(S, Mc)
            a.colsum = self.colsum.data_ptr()
            self.outs.append(self.colsum)
            self.checks.append(("column sums", lambda: self.colsum.sum(0, dtype=torch.float64), colref))
        n = ntap_out * Mc * Nc
        if S > 1:  # raw partial sums, slab by slab; fs2hip_reduce_slabs would add them
            self.result = [self.ws[:S * n]]
            self.checks.append(("sum of the slabs", lambda: self.ws[:S * n].view(S, ntap_out, Mc, Nc).sum(0, dtype=torch.float64), ref))
        else:
            self.result = [self.C]
            self.checks.append(("result", lambda: self.C, ref))
        self.result += [t for t in (self.pre, self.colsum) if t is not None]
        self.args = a

    def tolerance(self, ref, mode):
        """(scale of the error, bound): the fp32 kernels' relative 2e-5 (test_kernels_gpu.py), 4e-6 sqrt(K) + 1e-6 relative
        for operands rounded or split in registers (test_gemm_bf16_gpu.py, test_gemm_split_gpu.py), 4e-6 sqrt(K) of
        max(1, |ref|) for bf16 in memory (test_gemm_bf16_storage_gpu.py)"""
        K, top = self.c["R"], float(ref.abs().max())
        if mode == 0:
            return max(top, 1e-6), 2e-5
        if mode in (1, 2):
            return max(top, 1e-6), 4e-6 * math.sqrt(K) + 1e-6
        return 1.0, 4e-6 * math.sqrt(K) * max(1.0, top)

    def poison(self):
        for t in self.outs:
            t.fill_(float("nan"))

    def check(self, what):
        mode = self.c["mode"]
        for name, get, ref in self.checks:
            if self.ref_fp32 is not None and self.args.tile in STAGED:
                ref, mode = self.ref_fp32, 0
            got = get().detach().cpu().double().reshape(ref.shape)
            scale, tol = self.tolerance(ref, mode)
            err = float((got - ref).abs().max()) / scale
            print(f"{what} {name}: err {err:.3e} tol {tol:.3e}")
            assert err < tol, f"{what} {name}: err {err:.3e} > {tol:.3e}"

    def bytes(self):
        return b"".join(t.detach().cpu().contiguous().numpy().tobytes() for t in self.result)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def run_single(c, tile):
    if c["name"] not in BUILT:
        BUILT[c["name"]] = Built(c)
    b = BUILT[c["name"]]
    b.poison()
    b.args.tile = tile
    rc = H.real_lib().fs2hip_gemm(ctypes.byref(b.args), _stream())
    torch.cuda.synchronize()
    return rc, [b]


def group_members(name, orient, mode):
    if name not in BUILT:
        second = dict(Mc=72, Nc=64, R=96, seed=1)
        if orient == TN:
            second = dict(Mc=72, Nc=64, R=256, splitk=2, seed=1)
        BUILT[name] = [Built(case(name + "_0", orient, mode)), Built(case(name + "_1", orient, mode, **second))]
    return BUILT[name]


def run_group(name, orient, mode, tile):
    ms = group_members(name, orient, mode)
    for b in ms:
        b.poison()
    arr = (H.GemmArgs * len(ms))(*[b.args for b in ms])
    arr[0].tile = tile
    rc = H.real_lib().fs2hip_gemm_grouped(arr, len(ms), _stream())
    torch.cuda.synchronize()
    return rc, ms


BUILT = {}  # case name -> its tensors and references, built once and shared by every tile id


def digest(members):
    return hashlib.sha256(b"".join(b.bytes() for b in members)).hexdigest()[:12]


def sweep():
    """(case name, tile id, launcher) for every launch of the grid"""
    for c in CASES:
        for t in IDS:
            yield c["name"], t, (lambda c=c, t=t: run_single(c, t))
    for name, o, mode in GROUPS:
        for t in GROUP_IDS:
            yield name, t, (lambda name=name, o=o, mode=mode, t=t: run_group(name, o, mode, t))


def _verify(name, launches):
    want = json.loads(GOLDEN.read_text())[name]
    for tile, go in launches:
        rc_want, dg_want = want[str(tile)]
        rc, members = go()
        assert rc == rc_want, f"{name} tile {tile}: return code {rc}, recorded {rc_want}"
        if rc != 0:
            continue
        for b in members:
            b.check(f"{b.c['name']} tile {tile}")
        if dg_want is not None:
            assert digest(members) == dg_want, f"{name} tile {tile}: output bytes differ from the recorded launch"
    BUILT.pop(name, None)


@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_every_tile_id_accepts_refuses_and_computes_as_recorded(c):
    _verify(c["name"], [(t, (lambda t=t: run_single(c, t))) for t in IDS])


@pytest.mark.parametrize("name,orient,mode", GROUPS, ids=[g[0] for g in GROUPS])
def test_grouped_launches_accept_refuse_and_compute_as_recorded(name, orient, mode):
    _verify(name, [(t, (lambda t=t: run_group(name, orient, mode, t))) for t in GROUP_IDS])


def record(path):
    passes, failed = [], []
    for _ in range(2):
        got = {}
        for name, tile, go in sweep():
            rc, members = go()
            if rc == 0:
                try:
                    for b in members:
                        b.check(f"{name} tile {tile}")
                except AssertionError as e:
                    failed.append(str(e))
            got.setdefault(name, {})[str(tile)] = [rc, digest(members) if rc == 0 else None]
        passes.append(got)
    first, second = passes
    dropped = 0
    for name, tiles in first.items():
        for tile, (rc, dg) in tiles.items():
            assert second[name][tile][0] == rc, (name, tile)
            if second[name][tile][1] != dg:
                print(f"NOT REPRODUCED: {name} tile {tile}: {dg} then {second[name][tile][1]}; digest dropped")
                tiles[tile][1] = None
                dropped += 1
    Path(path).parent.mkdir(parents=True, exist_ok=True)
    Path(path).write_text(json.dumps(first, separators=(",", ":"), sort_keys=True).replace("},", "},\n") + "\n")
    n = sum(len(v) for v in first.values())
    ok = sum(1 for v in first.values() for rc, _ in v.values() if rc == 0)
    print(f"recorded {n} launches ({ok} accepted, {dropped} digests dropped) in {len(first)} cases -> {path}")
    assert not failed, "accepted launches off their float64 reference (do not commit this recording):\n" + "\n".join(failed)


if __name__ == "__main__":
    assert sys.argv[1:2] == ["--record"], "usage: python tests/test_gemm_dispatch_gpu.py --record [path]"
    record(sys.argv[2] if len(sys.argv) > 2 else GOLDEN)
