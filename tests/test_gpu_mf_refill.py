"""Scripted refill schedules replayed on the device against the numpy model (tests/mf_refill_model.py), kernel by
kernel: k_mf_stage_*, k_mf_publish, k_mf_drained, k_mf_decide (mf_plan), k_mf_update and k_mf_admit_rows are called
through their test entry points with the host's part of a series (when q_tail and drained move) as a deterministic
input. After every sweep MfState, MfQueue, X, Xprev, the output ring, xlast, xlast2, the recorded starts, ghat, arow
and O are compared with the model bit for bit (an extrapolated start: 1 ulp), and the device's own state goes through
the independent checker (I1 .. I5). The first difference names the sweep and the field.

Shapes: ld = 192 (three 64-voxel blocks), 131 voxels (the last block holds a partial quad of 3 and whole quads past the
shard), 77 rows padded to 128, 16 and 128 frames (both ballot words, the 128-column tile). The element-wise glue
(k_mf_weights, k_mf_collect, k_mf_penalty) follows at 16 .. 128 frames."""
from types import SimpleNamespace

import numpy as np
import pytest
from mf_refill_model import (F32, SRC_SLOT, bp_slot, cases, decode, decode_log, first_difference, replay, schedules)

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

# Largest relative deviation of the single-frame update_log kernel (powf, expf: device libm) from the fp64 formula on
# the operands of these schedules, measured once on an MI355X: 2.48e-07 (2.1 x 2^-23). The bound is twice that.
UPDATE_LOG_DEV = 2.48e-07
_measured = {"update_log": 0.0}


def _hip():
    from mpi_cuda_sartsolver_amd.ops import hip
    return hip()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _host(t):
    return t.cpu().numpy()


class DeviceReplay:
    """The device side of mf_refill_model.replay: every step runs the kernel and compares with the model."""

    def __init__(self, name):
        self.name, self.hip = name, _hip()
        self.SL, self.QL = self.hip.mf_state_layout(), self.hip.mf_queue_layout()
        self.stream = 0

    def fail(self, where, what):
        raise AssertionError(f"{self.name}: {where}: {what}")

    def begin(self, p, m, ray, dinv):
        h, self.p, self.m = self.hip, p, m
        z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device="cuda:0")  # noqa: E731
        nf, ld = p.nf, p.ld
        self.st, self.q = z(self.SL["nbytes"], dt=torch.uint8), z(self.QL["nbytes"], dt=torch.uint8)
        self.X, self.Xprev, self.O, self.D = z(nf, ld), z(nf, ld), z(ld, nf), z(ld, nf)
        self.pen, self.F2 = z(nf, ld), z(nf)
        self.ring, self.xlast, self.xlast2 = z(p.rcap, ld), z(ld), z(ld)
        self.starts = z(max(p.nframes, 1), ld)
        self.ghat, self.arow = z(p.nrows_pad, nf), z(p.nrows_pad, nf)
        self.g64q, self.ghq = z(p.qcap, p.nrows_pad, dt=torch.float64), z(p.qcap, p.nrows_pad)
        self.x0q, self.oq = z(p.qcap, ld), z(p.qcap, ld)
        self.stats, self.gpos, self.wo = z(2 * nf, dt=torch.float64), z(p.nrows_pad, nf), z(p.nrows_pad, nf)
        self.Dc = z(ld, nf)
        self.ray, self.dinv = _dev(ray), _dev(dinv)
        self.x0 = _dev(m.x0) if m.x0 is not None else None
        self.sink = z(1, dt=torch.int32)
        self.sst = z(h.state_nbytes(), dt=torch.uint8)  # a running single-frame state (done = 0)
        G0 = z(h.mf_max_frames(), dt=torch.float64)
        h.mf_state_begin(self.st.data_ptr(), G0.data_ptr(), 0, p.tol, p.max_iter, nf, self.stream)
        h.mf_queue_begin(self.q.data_ptr(), p.qcap, p.rcap, bool(p.chain), p.admit_cap, p.src_age, p.x0_below,
                         bool(p.src_finished), bool(p.lead), float(p.src_extrap), float(p.drift), self.stream)
        self.compare_structs(m, "begin")

    def structs(self):
        raw = _host(self.q)
        return decode(_host(self.st), self.SL), decode(raw, self.QL), decode_log(raw, self.QL)

    def compare_structs(self, m, where):
        st, q, log = self.structs()
        for ns, got, layout in ((m.st, st, self.SL["fields"]), (m.q, q, self.QL["fields"]),
                                (m.log, log, self.QL["log"]["fields"])):
            d = first_difference(ns, got, list(layout))
            if d:
                self.fail(where, d)
        return st, q, log

    def compare(self, where, **arrays):
        for name, (want, got) in arrays.items():
            got = _host(got)
            if want.tobytes() != got.tobytes():
                i = np.flatnonzero(want.reshape(-1).view(np.uint32) != got.reshape(-1).view(np.uint32))
                idx = np.unravel_index(i[0], want.shape)
                self.fail(where, f"{name}{list(map(int, idx))}: model {want[idx]!r}, device {got[idx]!r} "
                                 f"({i.size} differ)")

    def stage(self, e0, k, Gk, stats, gpos, wo, Dc, Do):
        h, p, s = self.hip, self.p, self.stream
        where = f"stage [{e0}, {e0 + k})"
        for j in range(k):
            self.g64q[(e0 + j) % p.qcap, :p.nrows] = _dev(Gk[j])
        h.mf_stage_stats(self.g64q.data_ptr(), e0, p.qcap, k, p.nrows, p.nrows_pad, self.stats.data_ptr(), p.nf, s)
        got = _host(self.stats)
        for j in list(range(k)) + list(range(p.nf, p.nf + k)):
            if got[j].tobytes() != stats[j].tobytes():
                self.fail(where, f"stats[{j}]: model {stats[j]!r}, device {got[j]!r}")
        h.mf_stage_norm(self.q.data_ptr(), self.g64q.data_ptr(), self.ghq.data_ptr(), self.stats.data_ptr(), e0, e0,
                        bool(p.cold), k, p.nrows, p.nrows_pad, p.nf, s)
        h.mf_stage_ops(self.ghq.data_ptr(), e0, p.qcap, k, p.nrows, p.nrows_pad, self.ray.data_ptr(), p.len_thres,
                       self.gpos.data_ptr(), self.wo.data_ptr(), p.nf, s)
        if p.cold:
            self.Dc.copy_(_dev(Dc))
            h.mf_stage_cols(self.Dc.data_ptr(), self.dinv.data_ptr(), e0, p.qcap, k, p.nvox, p.ld, p.nf,
                            self.x0q.data_ptr(), s)
        if p.log:
            self.Dc.copy_(_dev(Do))
            h.mf_stage_cols(self.Dc.data_ptr(), 0, e0, p.qcap, k, p.nvox, p.ld, p.nf, self.oq.data_ptr(), s)
        self.compare(where, ghq=(self.m.ghq, self.ghq), gpos=(gpos, self.gpos), wo=(wo, self.wo),
                     x0q=(self.m.x0q, self.x0q), oq=(self.m.oq, self.oq))

    def publish(self, tail):
        self.hip.mf_publish(self.q.data_ptr(), tail, self.stream)

    def drained(self, d):
        self.hip.mf_drained(self.q.data_ptr(), d, self.stream)

    def update_rows(self, p):
        """The voxel update of the model's running slots by the single-frame kernels (update_linear / update_log): what
        k_mf_update must equal bit for bit; both are held to the fp64 formula (log: UPDATE_LOG_DEV)."""
        h = self.hip

        def fn(x, d, o, pen):
            n, nv = x.shape
            xd, dd, od = _dev(x), _dev(d), _dev(o)
            pd = _dev(pen) if pen is not None else None
            for i in range(n):
                off = i * nv * 4
                pp = pd.data_ptr() + off if pd is not None else 0
                if p.log:
                    h.update_log(xd.data_ptr() + off, od.data_ptr() + off, dd.data_ptr() + off, pp, float(p.alpha),
                                 nv, self.sst.data_ptr(), self.stream)
                else:
                    h.update_linear(xd.data_ptr() + off, dd.data_ptr() + off, pp, nv, self.sst.data_ptr(),
                                    self.stream)
            new = _host(xd)
            x64, pen64 = x.astype(np.float64), (0.0 if pen is None else pen.astype(np.float64))
            if p.log:
                ratio = (o + F32(1e-7)).astype(np.float64) / (d + F32(1e-7)).astype(np.float64)
                ref = x64 * ratio ** float(F32(p.alpha)) * np.exp(-pen64)
                dev = np.max(np.abs(new - ref) / np.maximum(np.abs(ref), 1e-300))
                _measured["update_log"] = max(_measured["update_log"], float(dev))
                assert dev <= 2 * UPDATE_LOG_DEV, f"update_log is {dev:.3e} from the fp64 formula"
            else:  # two fp32 additions, each rounded once: the same operations in numpy
                v = x + d
                if pen is not None:
                    v = v - pen
                assert np.array_equal(new, np.where(v > 0, v, F32(0))), "update_linear is not x + d - pen, clipped"
            return new
        return fn

    def sweep(self, sweep, F2, D, pen, m):
        h, p, s = self.hip, self.p, self.stream
        where = f"sweep {sweep}"
        self.F2.copy_(_dev(F2))
        self.D.copy_(_dev(D))
        if pen is not None:
            self.pen.copy_(_dev(pen))
        # LDS the kernels below never wrote reads as NaN (not as what the kernel before happened to leave there)
        h.lds_fill(0x7FC00000, self.sink.data_ptr(), s)
        h.mf_decide(self.st.data_ptr(), self.F2.data_ptr(), self.q.data_ptr(), s)
        h.mf_update(self.X.data_ptr(), self.D.data_ptr(), self.O.data_ptr(), self.pen.data_ptr() if p.pen else 0,
                    float(p.alpha), bool(p.log), p.nvox, p.ld, self.st.data_ptr(), p.nf, self.Xprev.data_ptr(),
                    self.q.data_ptr(), ring=self.ring.data_ptr(), xlast=self.xlast.data_ptr(),
                    xlast2=self.xlast2.data_ptr(), x0=self.x0.data_ptr() if self.x0 is not None else 0,
                    x0q=self.x0q.data_ptr() if p.cold else 0, oq=self.oq.data_ptr() if p.log else 0,
                    starts=self.starts.data_ptr(), stream=s)
        h.mf_admit_rows(self.q.data_ptr(), self.ghq.data_ptr(), p.nrows, p.nrows_pad, self.ray.data_ptr(),
                        p.len_thres, self.ghat.data_ptr(), self.arow.data_ptr(), p.nf, s)
        st, q, log = self.compare_structs(m, where)
        X, starts = _host(self.X), _host(self.starts)
        if q.src_live and q.src_extrap != 0 and not p.log:
            # starts extrapolated by fmaf (the model rounds twice): 1 ulp, then the model continues from the device's
            for f in range(p.nf):
                if q.adm_pos[f] >= 0 and q.adm_kind[f] == SRC_SLOT:
                    k = int(q.slot_frame[f])
                    ulp = np.abs(X[f].view(np.int32).astype(np.int64) - m.X[f].view(np.int32).astype(np.int64))
                    if ulp.max() > 1 or not np.array_equal(X[f], starts[k]):
                        self.fail(where, f"extrapolated start of frame {k} (slot {f}): {ulp.max()} ulp from the model")
                    m.X[f] = X[f]
                    m.starts[k] = X[f]
        self.compare(where, X=(m.X, self.X), Xprev=(m.Xprev, self.Xprev), ring=(m.ring, self.ring),
                     xlast=(m.xlast, self.xlast), xlast2=(m.xlast2, self.xlast2), starts=(m.starts, self.starts),
                     ghat=(m.ghat, self.ghat), arow=(m.arow, self.arow), O=(m.O, self.O))
        return SimpleNamespace(st=st, q=q, log=log, X=X, Xprev=_host(self.Xprev), ring=_host(self.ring),
                               xlast=_host(self.xlast), xlast2=_host(self.xlast2), starts=starts,
                               x0q=_host(self.x0q), x0=m.x0)


@pytest.mark.parametrize("name,nf,log", cases())
def test_refill_schedule(name, nf, log):
    sched = schedules(nf)[name]
    dev = DeviceReplay(f"{name}[nf={nf}, log={log}]")
    m, chk = replay(sched, nf, log, backend=dev)
    assert m.q.fin == sched.nframes
    if log:
        print(f"update_log: largest relative deviation from the fp64 formula so far {_measured['update_log']:.3e}")


# ---------------------------------------------------------------------------------------------------------------
# Element-wise glue

NROWS_PAD, LD, NVOX = 128, 192, 131


@pytest.mark.parametrize("nsplit", [1, 3])
@pytest.mark.parametrize("wplane", [0, 16])
@pytest.mark.parametrize("log", [False, True])
@pytest.mark.parametrize("nf", [16, 32, 64, 128])
def test_mf_weights(nf, log, wplane, nsplit):
    """W bitwise fp32 numpy in split order (both layouts), per-block F2part at 1e-12 of fp64 (at most 64 non-negative
    terms per sum), wmax the exact maximum over the finite weights."""
    h = _hip()
    rng = np.random.default_rng(nf + nsplit)
    Fs = (rng.random((nsplit, NROWS_PAD, nf)) - 0.2).astype(F32)
    ghat = (rng.random((NROWS_PAD, nf)) * 2 - 0.5).astype(F32)
    arow = (rng.random((NROWS_PAD, nf)) * 3).astype(F32)
    arow[rng.random(arow.shape) < 0.1] = 0
    arow[5, 3] = np.inf  # a non-finite weight: left out of wmax
    nb = h.mf_weights_num_blocks(NROWS_PAD)
    assert nb == 2
    dFs, dg, da = _dev(Fs), _dev(ghat), _dev(arow)
    W = torch.full((NROWS_PAD * nf,), -7.0, device="cuda:0")
    F2part = torch.full((nb, nf), -7.0, dtype=torch.float64, device="cuda:0")
    wmax = torch.full((nf,), 12345, dtype=torch.int32, device="cuda:0")
    h.mf_weights(dFs.data_ptr(), nsplit, NROWS_PAD, dg.data_ptr(), da.data_ptr(), log, W.data_ptr(),
                 F2part.data_ptr(), nf, 0, wmax=wmax.data_ptr(), wplane=wplane)
    F = np.zeros((NROWS_PAD, nf), F32)
    for s in range(nsplit):
        F = F + Fs[s]
    with np.errstate(invalid="ignore"):
        w = arow * F if log else arow * (ghat - F)
    if wplane == 0:
        want = np.empty_like(w)
        for f in range(nf):
            want[:, bp_slot(f, nf)] = w[:, f]
    else:
        want = np.ascontiguousarray(w.reshape(NROWS_PAD, nf // wplane, wplane).transpose(1, 0, 2))
    got = _host(W).reshape(want.shape)
    assert got.tobytes() == want.tobytes()
    ref = (F.astype(np.float64) ** 2).reshape(nb, 64, nf).sum(axis=1)
    np.testing.assert_allclose(_host(F2part), ref, rtol=1e-12, atol=0)
    fin = np.where(np.abs(w) <= F32(3.0e38), np.abs(w), F32(0))
    assert np.array_equal(_host(wmax).view(np.uint32), fin.max(axis=0).view(np.uint32))


@pytest.mark.parametrize("scaled", [False, True])
@pytest.mark.parametrize("nsplit", [1, 3])
@pytest.mark.parametrize("nf", [16, 32, 64, 128])
def test_mf_collect(nf, nsplit, scaled):
    """D bitwise (splits summed in order, then the voxel's scale) on a sub-range [v0, v1) and nothing outside it;
    F2out within 1 ulp of float32(fp64 sum) with a partial count that is no multiple of 1024."""
    h = _hip()
    rng = np.random.default_rng(nf * 7 + nsplit)
    v0, v1, nF2 = 3, 131, 1300
    part = (rng.random((nsplit, LD, nf)) - 0.3).astype(F32)
    scale = (rng.random(LD) + 0.5).astype(F32)
    F2part = rng.random((nF2, nf)) * 10.0
    dp, ds, dF = _dev(part), _dev(scale), _dev(F2part)
    D = torch.full((LD, nf), -7.0, device="cuda:0")
    F2out = torch.full((nf,), -7.0, device="cuda:0")
    h.mf_collect(dp.data_ptr(), nsplit, LD, v0, v1, ds.data_ptr() if scaled else 0, D.data_ptr(), dF.data_ptr(), nF2,
                 F2out.data_ptr(), nf, 0)
    acc = np.zeros((LD, nf), F32)
    for s in range(nsplit):
        acc = acc + part[s]
    if scaled:
        acc = acc * scale[:, None]
    want = np.full((LD, nf), F32(-7.0))
    want[v0:v1] = acc[v0:v1]
    assert _host(D).tobytes() == want.tobytes()
    ref = F2part.sum(axis=0).astype(F32)
    ulp = np.abs(_host(F2out).view(np.int32).astype(np.int64) - ref.view(np.int32).astype(np.int64))
    assert ulp.max() <= 1, ulp
    # without the partial sums no block touches F2out, and a range of one voxel writes that voxel only
    D.fill_(-7.0)
    F2out.fill_(-7.0)
    h.mf_collect(dp.data_ptr(), nsplit, LD, 191, 192, ds.data_ptr() if scaled else 0, D.data_ptr(), 0, 0, 0, nf, 0)
    want = np.full((LD, nf), F32(-7.0))
    want[191] = acc[191]
    assert _host(D).tobytes() == want.tobytes() and np.all(_host(F2out) == -7.0)


@pytest.mark.parametrize("logx", [False, True])
@pytest.mark.parametrize("nf", [16, 32, 64, 128])
def test_mf_penalty(nf, logx):
    """Every running frame's penalty equals the single-frame kernel's bit for bit; finished frames are left alone."""
    h = _hip()
    rng = np.random.default_rng(nf)
    n = NVOX
    counts = rng.integers(0, 6, n)
    counts[0], counts[-1] = 0, 5
    row_ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    col = rng.integers(0, n, row_ptr[-1]).astype(np.int32)
    val = (rng.random(row_ptr[-1]) - 0.5).astype(F32)
    X = np.zeros((nf, LD), F32)
    X[:, :n] = rng.random((nf, n)) + 0.01
    nused = nf - 3  # k_mf_state_begin: frames >= nused are done
    SL = h.mf_state_layout()
    st = torch.zeros(SL["nbytes"], dtype=torch.uint8, device="cuda:0")
    G0 = torch.zeros(h.mf_max_frames(), dtype=torch.float64, device="cuda:0")
    h.mf_state_begin(st.data_ptr(), G0.data_ptr(), nused, 1e-4, 10, nf, 0)
    done = decode(_host(st), SL).done
    assert list(done[:nf]) == [0] * nused + [1] * 3
    drp, dc, dv, dX = _dev(row_ptr), _dev(col), _dev(val), _dev(X)
    pen = torch.full((nf, LD), -7.0, device="cuda:0")
    h.mf_penalty(drp.data_ptr(), dc.data_ptr(), dv.data_ptr(), n, 0.37, logx, dX.data_ptr(), LD, pen.data_ptr(),
                 st.data_ptr(), nf, 0)
    one = torch.full((nf, LD), -7.0, device="cuda:0")
    sst = torch.zeros(h.state_nbytes(), dtype=torch.uint8, device="cuda:0")
    for f in range(nused):
        h.penalty(logx, drp.data_ptr(), dc.data_ptr(), dv.data_ptr(), n, 0.37, dX.data_ptr() + f * LD * 4,
                  one.data_ptr() + f * LD * 4, sst.data_ptr(), 0)
    got, want = _host(pen), _host(one)
    assert got.tobytes() == want.tobytes()
    assert np.all(got[nused:] == -7.0) and np.all(got[:, n:] == -7.0) and np.all(got[:nused, 0] == 0.0)
    # against the fp64 formula: fp32 fma chains of at most 5 terms of magnitude <= 0.5 |h(x)|
    hx = np.log(X[:, :n].astype(np.float64)) if logx else X[:, :n].astype(np.float64)
    ref = np.zeros((nused, n))
    for r in range(n):
        k = slice(row_ptr[r], row_ptr[r + 1])
        ref[:, r] = float(F32(0.37)) * (hx[:nused][:, col[k]] * val[k].astype(np.float64)).sum(axis=1)
    # (six roundings of partial sums and logf's 2 ulp per term, each against S = 5 * 0.5 * max |h(x)|: 10 half-ulps)
    bound = 12 * 2.0 ** -24 * 0.37 * 5 * 0.5 * np.abs(hx).max()
    assert np.abs(got[:nused, :n] - ref).max() <= bound
