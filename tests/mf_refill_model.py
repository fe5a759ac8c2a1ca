"""A plain numpy / Python model of the multi-frame refill (csrc/kernels/multiframe_glue.hip: k_mf_decide with
mf_plan, k_mf_update, k_mf_admit_rows, k_mf_stage_stats / k_mf_stage_norm / k_mf_stage_ops / k_mf_stage_cols), an
independent checker of what a refill must guarantee, and the scripted schedules both tests replay.

The model is sequential (one Python loop per slot), integers for the plan, Python floats / np.float64 for doubles and
np.float32 for the iterates: every value the kernels compute in fp32 additions or fp64 rescales is reproduced bit for
bit. No torch. The struct fields carry the names of MfState / MfQueue / MfFinish (sart_common.hpp); their offsets
come from the extension (mf_state_layout / mf_queue_layout), see decode()."""
from fractions import Fraction
from types import SimpleNamespace

import numpy as np

KMAX, QMAX = 128, 256  # kMfMaxFrames, kMfQueueMax
SRC_NONE, SRC_SLOT, SRC_LAST, SRC_HOSTX0, SRC_COLD = 0, 1, 2, 3, 4
SUCCESS, MAX_ITER = 0, -1
F32, F64 = np.float32, np.float64
EPS = F32(1e-7)


def bp_slot(f, nf):
    """mf_bp_slot: position of frame f inside a row of a back-projection operand."""
    return (f & 15) * (nf >> 4) + (f >> 4)


def params(**kw):
    p = dict(nf=16, ld=192, nvox=131, nrows=77, nrows_pad=128, qcap=64, rcap=64, log=False, chain=True, admit_cap=0,
             src_age=0, src_finished=False, lead=False, x0_below=0, src_extrap=0.0, drift=0.0, tol=1e-4, max_iter=12,
             alpha=1.0, len_thres=0.05, cold=False, pen=False, nframes=0)
    p.update(kw)
    return SimpleNamespace(**p)


def _bit(words, f):
    return (int(words[f >> 6]) >> (f & 63)) & 1


def _setbit(words, f, on):
    w = int(words[f >> 6])
    words[f >> 6] = (w | (1 << (f & 63))) if on else (w & ~(1 << (f & 63)))


def _fma64(a, b, c):
    """fma(a, b, c) in double, exactly rounded once (the device contracts a * b + c in the drift expressions)."""
    return float(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


def _inv_len(ray_length, thres):
    with np.errstate(divide="ignore"):
        return np.where(ray_length > F32(thres), F32(1) / ray_length, F32(0)).astype(F32)


class RefillModel:
    def __init__(self, p, x0=None):
        self.p = p
        nf, ld = p.nf, p.ld
        i4 = lambda n, v=0: np.full(n, v, np.int32)  # noqa: E731
        f8 = lambda n, v=0.0: np.full(n, v, F64)  # noqa: E731
        # k_mf_state_begin with nused = 0 and G = 0 (every slot empty and done), as MultiFrameEngine::series_once
        G0 = f8(KMAX, 1.0)
        G0[:nf] = 0.0
        self.st = SimpleNamespace(G=G0, conv_prev=f8(KMAX), conv=f8(KMAX), done=i4(KMAX, 1),
                                  status=i4(KMAX, MAX_ITER), iters=i4(KMAX, p.max_iter), sweep=0, max_iter=p.max_iter,
                                  all_done=1, nf=nf, flags=np.zeros(2, np.uint64), tol=p.tol,
                                  rollback=np.zeros(2, np.uint64), sweep0=i4(KMAX))
        # zeroed memory, then k_mf_queue_begin
        self.q = SimpleNamespace(
            q_head=0, q_tail=0, fin=0, drained=0, qcap=p.qcap, rcap=p.rcap, chain=int(p.chain), admit_cap=p.admit_cap,
            src_age=p.src_age, src_finished=int(p.src_finished), lead=int(p.lead), src_extrap=F32(p.src_extrap),
            src_live=0, x0_below=p.x0_below, n_ret=0, n_adm=0, upd_any=0, skip_bwd=0, xlast_frame=-1, xlast_iter=-1,
            xlast_slot=-1, xlast_norm=1.0, xlast2_frame=-1, drift_frame1=-1, drift_frame2=-1, xlast2_norm=1.0,
            drift_norm1=1.0, drift_norm2=1.0, drift=F32(p.drift), src_kind=SRC_NONE, src_slot=-1, src_frame=-1,
            src_iter=-1, src_norm=1.0, slot_frame=i4(KMAX, -1), slot_warm_from=i4(KMAX, -1),
            slot_warm_iter=i4(KMAX, -1), slot_warm_live=i4(KMAX), slot_norm=f8(KMAX, 1.0), ret_pos=i4(KMAX, -1),
            ret_prev=i4(KMAX), adm_pos=i4(KMAX, -1), adm_kind=i4(KMAX, SRC_NONE), q_frame=i4(QMAX), q_cold=i4(QMAX),
            q_norm=f8(QMAX), q_G=f8(QMAX))
        self.log = SimpleNamespace(frame=i4(QMAX), status=i4(QMAX), iters=i4(QMAX), flags=i4(QMAX),
                                   warm_from=i4(QMAX), warm_iter=i4(QMAX), warm_live=i4(QMAX), conv=f8(QMAX),
                                   norm=f8(QMAX))
        z = lambda *s: np.zeros(s, F32)  # noqa: E731
        self.X, self.Xprev = z(nf, ld), z(nf, ld)
        self.O = z(ld, nf)
        self.ring, self.xlast, self.xlast2 = z(p.rcap, ld), z(ld), z(ld)
        self.starts = z(max(p.nframes, 1), ld)
        self.ghat, self.arow = z(p.nrows_pad, nf), z(p.nrows_pad, nf)
        self.g64q, self.ghq = np.zeros((p.qcap, p.nrows_pad), F64), z(p.qcap, p.nrows_pad)
        self.x0q, self.oq = z(p.qcap, ld), z(p.qcap, ld)
        self.x0 = None if x0 is None else np.asarray(x0, F64)
        self.drift_uses = 0  # admissions whose start took the drift term
        self.plans = []  # one record per executed plan (what the schedules' path assertions read)

    # ---- staging (k_mf_stage_stats, k_mf_stage_norm, k_mf_stage_ops, k_mf_stage_cols)
    def stage_stats(self, e0, k):
        p = self.p
        assert p.nrows <= 1024  # one row per thread: no order of additions inside a thread to reproduce
        stats = np.zeros(2 * p.nf, F64)
        for j in range(k):
            g = self.g64q[(e0 + j) % p.qcap, :p.nrows]
            v = np.where(np.isfinite(g), g, -1.0)
            rm, rs = np.full(1024, -np.inf), np.zeros(1024)
            rm[:p.nrows] = v
            rs[:p.nrows] = np.where(v > 0, v * v, 0.0)
            w = 512
            while w > 0:  # the kernel's tree: element t takes t + w
                rm[:w] = np.fmax(rm[:w], rm[w:2 * w])
                rs[:w] = rs[:w] + rs[w:2 * w]
                w >>= 1
            stats[j], stats[p.nf + j] = rm[0], rs[0]
        return stats

    def stage_norm(self, stats, e0, frame0, cold, k):
        p, q = self.p, self.q
        for j in range(k):
            pos = (e0 + j) % p.qcap
            mx = float(stats[j])
            norm = mx if mx > 0 else 1.0
            G = float(stats[p.nf + j]) / (norm * norm)
            if not G > 0:
                G = 1.0
            q.q_norm[pos], q.q_G[pos], q.q_frame[pos], q.q_cold[pos] = norm, G, frame0 + j, int(cold)
            g = self.g64q[pos, :p.nrows]
            self.ghq[pos] = 0
            self.ghq[pos, :p.nrows] = (np.where(np.isfinite(g), g, -1.0) / norm).astype(F32)

    def stage_ops(self, e0, k, ray_length):
        """(gpos, wo) [nrows_pad][nf] in the back-projection layout of columns j < k."""
        p = self.p
        gpos, wo = np.zeros((p.nrows_pad, p.nf), F32), np.zeros((p.nrows_pad, p.nf), F32)
        inv = _inv_len(ray_length, p.len_thres)
        for j in range(k):
            gh = self.ghq[(e0 + j) % p.qcap, :p.nrows]
            a = np.where(gh >= 0, inv, F32(0))
            gpos[:p.nrows, bp_slot(j, p.nf)] = np.where(gh > 0, gh, F32(0))
            wo[:p.nrows, bp_slot(j, p.nf)] = a * gh
        return gpos, wo

    def stage_cols(self, D, dinv, e0, k, out):
        p = self.p
        for j in range(k):
            x = D[:, j].copy()
            if dinv is not None:
                x[:p.nvox] = np.maximum(x[:p.nvox] * dinv[:p.nvox], EPS)
                x[:p.nvox][np.isnan(x[:p.nvox])] = EPS
                x[p.nvox:] = 0
            out[(e0 + j) % p.qcap] = x

    def publish(self, q_tail):
        self.q.q_tail = q_tail

    def drained(self, d):
        if d > self.q.drained:
            self.q.drained = d

    # ---- k_mf_decide
    def decide(self, F2):
        st, q = self.st, self.q
        active = not st.all_done
        s = st.sweep
        alld = True
        if active:
            for f in range(st.nf):
                F = float(F2[f])
                sf = s - int(st.sweep0[f])
                done = int(st.done[f])
                if not np.isfinite(F):
                    if not done:
                        _setbit(st.flags, f, 1)
                        if sf > 0:
                            _setbit(st.rollback, f, 1)
                        st.iters[f] = sf - 1 if sf > 0 else 0
                        done = 1
                elif sf >= 1:
                    with np.errstate(all="ignore"):  # (a slot never filled has G = 0)
                        conv = float((st.G[f] - F64(F)) / st.G[f])
                    newly = (not done) and sf >= 2 and abs(conv - float(st.conv_prev[f])) < st.tol
                    if newly:
                        st.status[f], st.iters[f] = SUCCESS, sf
                    if not (done and not newly):
                        st.conv_prev[f] = conv
                    st.conv[f] = conv
                    done = 1 if (done or newly) else 0
                if sf >= st.max_iter:
                    done = 1
                st.done[f] = done
                if not done:
                    alld = False
            st.sweep = s + 1
        self._plan(s + 1 if active else s, active and not alld, active)

    # ---- mf_plan
    def _plan(self, sweep_new, ran, active):
        st, q, L = self.st, self.q, self.log
        nf = st.nf
        R = range(nf)
        fr = [int(q.slot_frame[f]) for f in R]
        occ = [fr[f] >= 0 for f in R]
        dn = [st.done[f] != 0 for f in R]
        nonfin = [_bit(st.flags, f) for f in R]
        rb = [_bit(st.rollback, f) for f in R]
        sw0 = [int(st.sweep0[f]) for f in R]
        upd = [sweep_new - sw0[f] for f in R]
        q.drift_frame1, q.drift_norm1 = q.xlast_frame, q.xlast_norm
        q.drift_frame2, q.drift_norm2 = q.xlast2_frame, q.xlast2_norm
        fin = q.fin
        room = q.rcap - (fin - q.drained)
        rank_fin, retire, n = [0] * nf, [False] * nf, 0
        for f in R:  # retire in slot order while the ring has room
            if occ[f] and dn[f]:
                rank_fin[f], retire[f] = n, n < room
                n += 1
        nret = n if n < room else max(room, 0)
        best = best_ret = -1
        for f in R:
            if q.chain and occ[f] and not nonfin[f] and (dn[f] or (not q.src_finished and upd[f] >= q.src_age)):
                best = max(best, fr[f])
            if retire[f] and not nonfin[f] and fr[f] > q.xlast_frame:
                best_ret = max(best_ret, fr[f])
        fre = [(not occ[f]) or retire[f] for f in R]
        s_kind, s_slot, s_iter, s_norm, s_live = SRC_NONE, -1, -1, 1.0, 0
        if q.chain and q.xlast_frame > best and q.xlast_frame >= 0:
            best = q.xlast_frame
            s_kind, s_iter, s_norm = SRC_LAST, q.xlast_iter, q.xlast_norm
        for f in R:
            if occ[f] and fr[f] == best:
                s_kind, s_slot, s_norm = SRC_SLOT, f, float(q.slot_norm[f])
                s_iter, s_live = (int(st.iters[f]), 0) if dn[f] else (upd[f], 1)
        xl = [f for f in R if retire[f] and fr[f] == best_ret]
        xl_new = (xl[0], fr[xl[0]], int(st.iters[xl[0]]), float(q.slot_norm[xl[0]])) if xl else None
        for f in R:
            if retire[f]:
                pos = (fin + rank_fin[f]) % q.rcap
                L.frame[pos] = fr[f]
                L.status[pos] = SUCCESS if st.status[f] == SUCCESS else MAX_ITER
                L.iters[pos] = st.iters[f]
                L.flags[pos] = (1 if nonfin[f] else 0) | (2 if rb[f] else 0)
                L.warm_from[pos], L.warm_iter[pos] = q.slot_warm_from[f], q.slot_warm_iter[f]
                L.warm_live[pos] = q.slot_warm_live[f]
                L.conv[pos], L.norm[pos] = st.conv[f], q.slot_norm[f]
                q.ret_pos[f], q.ret_prev[f], q.slot_frame[f] = pos, 1 if rb[f] else 0, -1
            else:
                q.ret_pos[f] = -1
        xlast_before = q.xlast_frame
        if xl_new:
            q.xlast2_frame, q.xlast2_norm = q.xlast_frame, q.xlast_norm
            q.xlast_slot, q.xlast_frame, q.xlast_iter, q.xlast_norm = xl_new
        avail = q.q_tail - q.q_head
        nfree = sum(fre)
        nadm = nfree
        if q.admit_cap > 0 and nadm > q.admit_cap:
            nadm = q.admit_cap
        if q.lead and best_ret < 0 and xlast_before < 0:
            nadm = 1 if (nfree == nf and nadm > 0) else 0
        if nadm > avail:
            nadm = avail
        adm, n = [False] * nf, 0
        for f in R:
            if fre[f]:
                if n < nadm:
                    adm[f] = True
                    pos = (q.q_head + n) % q.qcap
                    frame = int(q.q_frame[pos])
                    kind = SRC_NONE
                    if q.chain and s_kind != SRC_NONE:
                        kind = s_kind
                    elif frame < q.x0_below:
                        kind = SRC_HOSTX0
                    elif q.q_cold[pos]:
                        kind = SRC_COLD
                    chained = kind in (SRC_SLOT, SRC_LAST)
                    q.adm_pos[f], q.adm_kind[f], q.slot_frame[f], q.slot_norm[f] = pos, kind, frame, q.q_norm[pos]
                    q.slot_warm_from[f] = best if chained else -1
                    q.slot_warm_iter[f] = s_iter if chained else -1
                    q.slot_warm_live[f] = s_live if (chained and s_kind == SRC_SLOT) else 0
                    st.G[f], st.conv_prev[f], st.conv[f], st.done[f] = q.q_G[pos], 0.0, 0.0, 0
                    st.status[f], st.iters[f], st.sweep0[f] = MAX_ITER, st.max_iter, sweep_new
                    _setbit(st.flags, f, 0)
                    _setbit(st.rollback, f, 0)
                n += 1
            if not adm[f]:
                q.adm_pos[f] = -1
        run_next = [adm[f] or (occ[f] and not dn[f]) for f in R]
        nrun = sum(run_next)
        nmax = sum(1 for f in R if run_next[f] and not adm[f] and sweep_new - sw0[f] >= st.max_iter)
        q.fin, q.q_head, q.n_ret, q.n_adm, q.upd_any = fin + nret, q.q_head + nadm, nret, nadm, 1 if ran else 0
        q.src_kind, q.src_slot, q.src_frame, q.src_iter, q.src_norm, q.src_live = (s_kind, s_slot, best, s_iter,
                                                                                   s_norm, s_live)
        if best_ret < 0:
            q.xlast_slot = -1
        st.all_done = 1 if nrun == 0 else 0
        q.skip_bwd = 1 if (nrun == 0 or nmax == nrun) else 0
        self.plans.append(SimpleNamespace(
            idle=not active, n_ret=nret, n_adm=nadm, kinds=[int(q.adm_kind[f]) for f in R if adm[f]],
            waiting=sum(1 for f in R if occ[f] and dn[f] and not retire[f]), src_kind=s_kind, src_live=s_live,
            src_waiting=s_kind == SRC_SLOT and dn[s_slot] and not retire[s_slot], words=(sum(adm[:64]), sum(adm[64:])),
            ret_words=(sum(retire[:64]), sum(retire[64:])), ret_prev=sum(1 for f in R if retire[f] and rb[f]),
            skip_bwd=int(q.skip_bwd), head=int(q.q_head), nmax=nmax, xlast_moved=xl_new is not None))

    # ---- k_mf_update
    @staticmethod
    def update_rows_numpy(log, alpha):
        """The voxel update in numpy fp32 (linear: exact; log: libm's powf / expf, not the device's)."""
        def fn(x, d, o, pen):
            if log:
                r = np.power((o + EPS) / (d + EPS), F32(alpha), dtype=F32)
                if pen is not None:
                    r = r * np.exp(-pen, dtype=F32)
                return (x * r).astype(F32)
            v = x + d
            if pen is not None:
                v = v - pen
            return np.where(v > 0, v, F32(0)).astype(F32)
        return fn

    def update(self, D, pen=None, update_rows=None):
        """D [ld][nf] (and self.O in log mode), pen [nf][ld] or None. update_rows(x, d, o, pen) -> x' on [n][nvox]
        operands of the running slots (default: numpy)."""
        p, st, q = self.p, self.st, self.q
        nf, nv = p.nf, p.nvox
        refill = bool(q.n_ret or q.n_adm or q.xlast_slot >= 0)
        if not q.upd_any and not refill:
            return
        if q.upd_any:
            run = [f for f in range(nf) if not st.done[f] and q.adm_pos[f] < 0]
            if run:
                fn = update_rows or self.update_rows_numpy(p.log, p.alpha)
                x = self.X[run, :nv]
                new = fn(x, np.ascontiguousarray(D[:nv, run].T), np.ascontiguousarray(self.O[:nv, run].T),
                         None if pen is None else pen[run, :nv])
                self.Xprev[run, :nv] = x
                self.X[run, :nv] = new
        if not refill:
            return
        use_drift = (q.n_adm > 0 and q.drift != 0 and not p.log and q.drift_frame2 >= 0
                     and q.drift_frame1 > q.drift_frame2)
        drift_s = np.zeros(p.ld, F32)
        if use_drift:
            for v in range(nv):  # (double)xlast n1 - (double)xlast2 n2, contracted: fma(xlast, n1, -(xlast2 n2))
                t = float(self.xlast2[v]) * q.drift_norm2
                drift_s[v] = F32(_fma64(self.xlast[v], q.drift_norm1, -t) / float(q.drift_frame1 - q.drift_frame2))
        cx = q.src_extrap if (q.src_live and not p.log) else F32(0)
        new = {}
        assert not (q.xlast_slot >= 0 and SRC_LAST in [int(q.adm_kind[f]) for f in range(nf) if q.adm_pos[f] >= 0])
        for f in range(nf):
            ap = int(q.adm_pos[f])
            if ap < 0:
                continue
            kind, s_new = int(q.adm_kind[f]), float(q.slot_norm[f])
            chained = kind in (SRC_SLOT, SRC_LAST)
            x = np.zeros(p.ld, F32)
            if chained:
                xs = (self.X[q.src_slot, :nv] if kind == SRC_SLOT else self.xlast[:nv]).copy()
                if kind == SRC_SLOT and cx != 0:  # fmaf(cx, xs - xprev, xs), here rounded twice (<= 1 ulp off)
                    dx = xs - self.Xprev[q.src_slot, :nv]
                    xs = (F64(cx) * dx.astype(F64) + xs.astype(F64)).astype(F32)
                if use_drift:
                    self.drift_uses += 1
                    dgap = q.drift * F32(int(q.slot_frame[f]) - q.src_frame)
                    t = (dgap * drift_s[:nv]).astype(F64)
                    sc = np.array([_fma64(a, q.src_norm, b) for a, b in zip(xs, t)], F64)
                else:
                    sc = xs.astype(F64) * q.src_norm
                x[:nv] = (sc / s_new).astype(F32)
            elif kind == SRC_HOSTX0:
                x[:nv] = (self.x0[:nv] / s_new).astype(F32)
            elif kind == SRC_COLD:
                x[:nv] = self.x0q[ap, :nv]
            x[:nv] = np.where(x[:nv] > EPS, x[:nv], EPS)
            new[f] = x
            if p.log:
                self.O[:, f] = self.oq[ap]
        for f in range(nf):  # retired iterates into the ring and xlast (before the admitted slots are overwritten)
            rp = int(q.ret_pos[f])
            if rp >= 0 or f == q.xlast_slot:
                val = (self.Xprev if (rp >= 0 and q.ret_prev[f]) else self.X)[f].copy()
                if rp >= 0:
                    self.ring[rp] = val
                if f == q.xlast_slot:
                    self.xlast2[:] = self.xlast
                    self.xlast[:] = val
        for f, x in new.items():
            self.X[f] = x
            self.starts[int(q.slot_frame[f])] = x

    # ---- k_mf_admit_rows
    def admit_rows(self, ray_length):
        p, q = self.p, self.q
        if q.n_adm == 0:
            return
        inv = _inv_len(ray_length, p.len_thres)
        for f in range(p.nf):
            pos = int(q.adm_pos[f])
            if pos >= 0:
                gh = self.ghq[pos, :p.nrows]
                self.ghat[:, f], self.arow[:, f] = 0, 0
                self.ghat[:p.nrows, f] = gh
                self.arow[:p.nrows, f] = np.where(gh >= 0, inv, F32(0))

    def snapshot(self):
        c = lambda ns: SimpleNamespace(**{k: (v.copy() if isinstance(v, np.ndarray) else v)  # noqa: E731
                                          for k, v in vars(ns).items()})
        return SimpleNamespace(st=c(self.st), q=c(self.q), log=c(self.log), X=self.X.copy(), Xprev=self.Xprev.copy(),
                               ring=self.ring.copy(), xlast=self.xlast.copy(), xlast2=self.xlast2.copy(),
                               starts=self.starts.copy(), x0q=self.x0q, x0=self.x0)


def decode(raw, layout):
    """Raw device bytes of a struct -> namespace of its fields by the extension's layout (count 1: a scalar)."""
    raw = np.frombuffer(bytes(raw), np.uint8)
    out = {}
    for name, (off, dt, cnt) in layout["fields"].items():
        a = np.frombuffer(raw, np.dtype(dt), cnt, off).copy()
        out[name] = a if cnt > 1 else a[0]
    return SimpleNamespace(**out)


def decode_log(raw, layout):
    """The MfFinish array of raw MfQueue bytes -> namespace of per-position field arrays."""
    lg = layout["log"]
    raw = np.frombuffer(bytes(raw), np.uint8)
    recs = raw[lg["offset"]:lg["offset"] + lg["count"] * lg["nbytes"]].reshape(lg["count"], lg["nbytes"])
    out = {}
    for name, (off, dt, cnt) in lg["fields"].items():
        out[name] = np.ascontiguousarray(recs[:, off:off + np.dtype(dt).itemsize]).view(np.dtype(dt)).reshape(-1)
    return SimpleNamespace(**out)


def first_difference(model_ns, got_ns, names):
    """Name of the first field whose bytes differ (None: all equal); every name must exist on both sides."""
    for name in names:
        g = np.asarray(getattr(got_ns, name))
        m = np.asarray(getattr(model_ns, name)).astype(g.dtype)
        if m.tobytes() != g.tobytes():
            bad = [i for i in range(m.size) if m.reshape(-1)[i:i + 1].tobytes() != g.reshape(-1)[i:i + 1].tobytes()]
            i = bad[0]
            return f"{name}[{i}]: model {m.reshape(-1)[i]!r}, device {g.reshape(-1)[i]!r} ({len(bad)} differ)"
    return None


# ---------------------------------------------------------------------------------------------------------------
# The independent checker: it never calls the plan model. It is fed the state after every sweep (the device's own, or
# the model's in the CPU test), keeps each frame's iterate by update count from the X it sees, and asserts I1 .. I5.
class ChainChecker:
    def __init__(self, p):
        self.p = p
        self.hist, self.norm = {}, {}  # frame -> [iterate after 0, 1, .. updates]; frame -> its normalisation
        self.admitted, self.retired = {}, {}  # frame -> times
        self.slot = [-1] * p.nf
        self.prev = None
        self.ever_live = False
        self.sweep = 0

    def after_sweep(self, s):
        p, st, q, L = self.p, s.st, s.q, s.log
        nf, nv = p.nf, p.nvox
        where = f"sweep {self.sweep}"
        # updates of the slots that kept their frame and ran
        if q.upd_any:
            for f in range(nf):
                if self.slot[f] >= 0 and q.slot_frame[f] == self.slot[f] and not st.done[f] and q.adm_pos[f] < 0:
                    self.hist[self.slot[f]].append(s.X[f].copy())
        # I2: retirements
        for f in range(nf):
            pos = int(q.ret_pos[f])
            if pos < 0:
                continue
            frame = self.slot[f]
            assert frame >= 0 and L.frame[pos] == frame, f"I1 {where}: slot {f} retires {L.frame[pos]}, held {frame}"
            self.retired[frame] = self.retired.get(frame, 0) + 1
            it = int(L.iters[pos])
            assert 0 <= it < len(self.hist[frame]), f"I2 {where}: frame {frame} reports {it} updates"
            want = self.hist[frame][it]
            assert bool(L.flags[pos] & 2) == (it == len(self.hist[frame]) - 2 and bool(L.flags[pos] & 1)), \
                f"I2 {where}: frame {frame} rollback bit"
            if L.flags[pos] & 2:
                assert q.ret_prev[f] == 1, f"I2 {where}: ret_prev of slot {f}"
                assert self.prev.Xprev[f].tobytes() == want.tobytes(), f"I2 {where}: Xprev of slot {f}"
            assert s.ring[pos].tobytes() == want.tobytes(), f"I2 {where}: ring row {pos} of frame {frame}"
            assert L.norm[pos] == self.norm[frame], f"I2 {where}: norm of frame {frame}"
            self.slot[f] = -1
        # I3 / I4: admissions
        for f in range(nf):
            ap = int(q.adm_pos[f])
            if ap < 0:
                continue
            frame = int(q.slot_frame[f])
            assert self.slot[f] < 0, f"I1 {where}: slot {f} admitted while it holds frame {self.slot[f]}"
            self.admitted[frame] = self.admitted.get(frame, 0) + 1
            wf, wi, wl = int(q.slot_warm_from[f]), int(q.slot_warm_iter[f]), int(q.slot_warm_live[f])
            kind, s_new = int(q.adm_kind[f]), float(q.slot_norm[f])
            self.norm[frame] = s_new
            x = np.zeros(p.ld, F32)
            tol_ulp = 0
            if wf < 0:
                assert kind in (SRC_NONE, SRC_HOSTX0, SRC_COLD), f"I3 {where}: frame {frame} kind {kind}"
                if kind == SRC_HOSTX0:
                    x[:nv] = (s.x0[:nv] / s_new).astype(F32)
                elif kind == SRC_COLD:
                    x[:nv] = s.x0q[ap, :nv]
            else:
                assert kind in (SRC_SLOT, SRC_LAST), f"I3 {where}: frame {frame} kind {kind}"
                assert wf < frame, f"I4 {where}: frame {frame} chained from {wf}"
                assert wf in self.hist and 0 <= wi < len(self.hist[wf]), f"I3 {where}: source {wf} at {wi} updates"
                assert q.src_norm == self.norm[wf], f"I3 {where}: src_norm {q.src_norm} of frame {wf}"
                src = self.hist[wf][wi][:nv]
                if wl:
                    self.ever_live = True
                    assert wi >= q.src_age, f"I4 {where}: live source {wf} has {wi} < src_age updates"
                    assert wi == len(self.hist[wf]) - 1 and self.retired.get(wf, 0) == 0, f"I4 {where}: {wf} not live"
                    if q.src_extrap != 0 and not p.log:
                        assert wi >= 1
                        src = (F64(q.src_extrap) * (src - self.hist[wf][wi - 1][:nv]).astype(F64)
                               + src.astype(F64)).astype(F32)
                        tol_ulp = 1
                t = np.zeros(nv, F64)
                if (q.drift != 0 and not p.log and q.drift_frame2 >= 0 and q.drift_frame1 > q.drift_frame2):
                    d = np.array([F32(_fma64(a, q.drift_norm1, -(float(b) * q.drift_norm2))
                                      / float(q.drift_frame1 - q.drift_frame2))
                                  for a, b in zip(self.prev.xlast[:nv], self.prev.xlast2[:nv])], F32)
                    t = ((q.drift * F32(frame - wf)) * d).astype(F64)
                    x[:nv] = (np.array([_fma64(a, q.src_norm, b) for a, b in zip(src, t)], F64) / s_new).astype(F32)
                else:
                    x[:nv] = (src.astype(F64) * q.src_norm / s_new).astype(F32)
            x[:nv] = np.where(x[:nv] > EPS, x[:nv], EPS)
            got = s.starts[frame]
            if tol_ulp:
                d = np.abs(got.view(np.int32).astype(np.int64) - x.view(np.int32).astype(np.int64))
                assert d.max() <= tol_ulp, f"I3 {where}: start of frame {frame} {d.max()} ulp from its source"
            else:
                assert got.tobytes() == x.tobytes(), f"I3 {where}: start of frame {frame} is not its source {wf}@{wi}"
            assert s.X[f].tobytes() == got.tobytes(), f"I3 {where}: X of slot {f} is not the recorded start"
            self.hist[frame] = [got.copy()]
            self.slot[f] = frame
        assert [int(v) for v in q.slot_frame[:nf]] == self.slot, f"I1 {where}: slot table"
        if q.src_finished:
            assert not self.ever_live, f"I4 {where}: a live source with src_finished"
        # I5
        assert q.q_head <= q.q_tail, f"I5 {where}: q_head {q.q_head} > q_tail {q.q_tail}"
        assert 0 <= q.fin - q.drained <= q.rcap, f"I5 {where}: fin {q.fin} drained {q.drained}"
        runs = any(self.slot[f] >= 0 and not st.done[f] for f in range(nf))
        assert bool(st.all_done) == (not runs), f"I5 {where}: all_done {st.all_done}, a slot runs: {runs}"
        self.prev = s
        self.sweep += 1

    def finish(self, published):
        """I1 over the whole series (published: the frame ids made visible to the plan)."""
        for k in published:
            assert self.admitted.get(k, 0) == 1, f"I1: frame {k} admitted {self.admitted.get(k, 0)} times"
            assert self.retired.get(k, 0) == 1, f"I1: frame {k} retired {self.retired.get(k, 0)} times"
        assert set(self.admitted) == set(published) == set(self.retired), "I1: frames outside the published set"


# ---------------------------------------------------------------------------------------------------------------
# Schedules. A schedule fixes the parameters, the frames' lifetimes and, per sweep, what the host does before the
# sweep (publish up to, drained up to). Everything else follows from the plan.
class Schedule:
    def __init__(self, name, nframes, life=None, nan_at=None, x0=False, **kw):
        self.name, self.nframes, self.kw, self.x0 = name, nframes, kw, x0
        self.life = life or (lambda k: 2 + (k * 7 + 3) % 5)  # own sweep at which frame k's convergence repeats
        self.nan_at = nan_at or {}  # frame -> own sweep of a NaN in ||A x||^2

    def params(self, nf, log):
        # (log mode: a relaxation that makes powf work)
        return params(nf=nf, log=log, nframes=self.nframes, alpha=0.75 if log else 1.0, **{k: (v(nf) if callable(v) else v)
                                                               for k, v in self.kw.items() if k not in HOST_KEYS})

    def host(self, key, default):
        return self.kw.get(key, default)


HOST_KEYS = ("publish", "drain", "linear_only")  # keys of a schedule that are not kernel parameters


def make_F2(model, sched, rng):
    """||A x||^2 of this sweep per slot, from the model's slot table: frame k's convergence value changes by more
    than tol every sweep until its own sweep L_k, where it repeats (so the frame converges there); None: never."""
    st, q, nf = model.st, model.q, model.p.nf
    F2 = (rng.random(nf) + 0.5).astype(F32)  # empty and finished slots: any finite value
    for f in range(nf):
        k = int(q.slot_frame[f])
        if k < 0 or st.done[f]:
            continue
        sf = st.sweep - int(st.sweep0[f])
        L = sched.life(k)
        step = sf - 1 if (L is not None and sf >= L) else sf
        F2[f] = F32(float(st.G[f]) * (0.5 + 0.3 / (step + 1.0)))
        if sched.nan_at.get(k) == sf:
            F2[f] = np.nan
    return F2


def pixels(rng, nframes, nrows):
    """Raw fp64 pixels: positive values of different scales per frame, some saturated (-1) and one non-finite."""
    g = rng.random((nframes, nrows)) * (1.0 + rng.random((nframes, 1)) * 50.0)
    g[rng.random(g.shape) < 0.05] = -1.0
    g[0, 5] = np.inf
    return g


def host_script(sched, nf):
    """(publish(sweep, tail, state) -> new tail, drain(sweep, drained, fin) -> new drained)."""
    n = sched.nframes
    pub = sched.host("publish", lambda sweep, tail, q, st, nf: n)
    drn = sched.host("drain", lambda sweep, drained, fin: fin)
    return pub, drn


def _lagging(sweep, tail, q, st, nf):
    return tail + (1 + sweep % 3 if sweep % 2 == 0 else 0)


def _starved(sweep, tail, q, st, nf):  # a new burst only after a plan that ran alone and had nothing to do
    idle = st.all_done and q.q_head == tail and q.n_adm == 0 and q.n_ret == 0
    return tail + (1 + (tail * 5) % 3) if idle else tail


def _lag_drain(sweep, drained, fin):  # the host copies one ring entry out every second sweep
    return drained + (1 if (sweep % 2 == 1 and drained < fin) else 0)


def schedules(nf):
    q4 = max(1, nf // 4)
    S = [
        Schedule("steady", 3 * nf, pen=True, qcap=min(QMAX, 4 * nf), rcap=min(QMAX, 4 * nf)),
        Schedule("lagging", nf + 9, publish=_lagging),
        Schedule("starved", 11, publish=_starved),
        Schedule("ring_pressure", nf + 21, rcap=4, src_finished=True, drain=_lag_drain, qcap=min(QMAX, 4 * nf)),
        Schedule("queue_wrap", 3 * 8 + 5, qcap=8,
                 publish=lambda sweep, tail, q, st, nf: min(tail + 3, int(q.q_head) + 8)),
        Schedule("nonfinite", nf + 6, nan_at={0: 0, 2: 3, nf + 1: 0, nf + 3: 2}, publish=_lagging),
        Schedule("max_iter", nf + 3, life=lambda k: None if k % 3 else 2 + k % 4, max_iter=6,
                 publish=lambda sweep, tail, q, st, nf: nf if q.fin < nf else 10 ** 9),
        Schedule("knobs_cap1_age3", nf + 7, admit_cap=1, src_age=3, life=lambda k: 5 + k % 4),
        Schedule("knobs_capq_age0", 2 * nf, admit_cap=q4, src_age=0),
        Schedule("knobs_src_finished", nf + 7, admit_cap=q4, src_finished=True, publish=_lagging),
        Schedule("knobs_lead", nf + 5, lead=True, cold=True, admit_cap=q4, src_age=1),
        Schedule("knobs_nochain_x0", nf + 9, chain=False, x0=True, x0_below=nf, cold=True,
                 qcap=min(QMAX, 4 * nf), rcap=min(QMAX, 4 * nf)),
        Schedule("knobs_nochain_cold", nf + 4, chain=False, cold=True, qcap=min(QMAX, 4 * nf), rcap=min(QMAX, 4 * nf)),
        Schedule("knobs_chain_x0", nf + 6, x0=True, x0_below=2 ** 40, admit_cap=q4, src_age=3),
        Schedule("knobs_extrap4", nf + 9, src_extrap=4.0, admit_cap=q4, src_age=3, life=lambda k: 5 + k % 3,
                 linear_only=True),
        Schedule("knobs_drift1", nf + 9, drift=1.0, admit_cap=q4, src_age=1, publish=_lagging, linear_only=True),
    ]
    for s in S:
        s.kw.setdefault("qcap", min(QMAX, 4 * nf))
        s.kw.setdefault("rcap", min(QMAX, 4 * nf))
    return {s.name: s for s in S}



def cases():
    """(schedule, nf, log) of both tests: every schedule at 16 and 128 frames, linear and log mode (extrapolation and
    drift exist in linear mode only)."""
    return [(name, nf, log) for nf in (16, 128) for name, s in schedules(nf).items() for log in (False, True)
            if not (log and s.kw.get("linear_only"))]


def replay(sched, nf, log, seed=0, backend=None, max_sweeps=700):
    """Run a schedule through the model (and, with a backend, through the device after every step; the backend
    compares and raises at the first difference). Returns (model, checker, published frame ids)."""
    p = sched.params(nf, log)
    rng = np.random.default_rng(seed + nf)
    x0 = (rng.random(p.nvox) * 40.0 + 0.01) if sched.x0 else None
    m = RefillModel(p, x0)
    chk = ChainChecker(p)
    G = pixels(rng, sched.nframes, p.nrows)
    ray = (rng.random(p.nrows_pad) * 2.0).astype(F32)  # some rows below len_thres
    ray[:4] = [0.0, 0.01, 0.05, 0.0500001]
    dinv = (rng.random(p.ld) + 0.2).astype(F32)
    if backend:
        backend.begin(p, m, ray, dinv)
    pub, drn = host_script(sched, nf)
    tail = drained = 0
    for sweep in range(max_sweeps):
        new_tail = min(sched.nframes, pub(sweep, tail, m.q, m.st, nf))
        new_tail = min(new_tail, m.q.q_head + p.qcap)  # (the host never overwrites an entry not yet admitted)
        while tail < new_tail:  # stage in units of at most nf entries, as MultiFrameEngine::stage
            k = min(nf, new_tail - tail)
            for j in range(k):
                m.g64q[(tail + j) % p.qcap, :p.nrows] = G[tail + j]
            stats = m.stage_stats(tail, k)
            m.stage_norm(stats, tail, tail, p.cold, k)
            gpos, wo = m.stage_ops(tail, k, ray[:p.nrows])
            Dc = (rng.random((p.ld, nf)) * 3.0 - 0.1).astype(F32)  # stands for the reduced back-projections
            Do = (rng.random((p.ld, nf)) + 0.1).astype(F32)
            if p.cold:
                m.stage_cols(Dc, dinv, tail, k, m.x0q)
            if p.log:
                m.stage_cols(Do, None, tail, k, m.oq)
            if backend:
                backend.stage(tail, k, G[tail:tail + k], stats, gpos, wo, Dc, Do)
            tail += k
            m.publish(tail)
            if backend:
                backend.publish(tail)
        d = drn(sweep, drained, int(m.q.fin))
        if d != drained:
            drained = d
            m.drained(d)
            if backend:
                backend.drained(d)
        F2 = make_F2(m, sched, rng)
        D = (rng.random((p.ld, nf)) * 0.2 - 0.05 + (0.9 if log else 0.0)).astype(F32)
        pen = (rng.random((nf, p.ld)) * 0.02).astype(F32) if p.pen else None
        m.decide(F2)
        m.update(D, pen, backend.update_rows(p) if backend else None)
        m.admit_rows(ray[:p.nrows])
        snap = m.snapshot()
        if backend:
            snap = backend.sweep(sweep, F2, D, pen, m)  # compares everything; returns the device's own state
        chk.after_sweep(snap)
        if m.q.fin == sched.nframes and tail == sched.nframes:
            break
    else:
        raise AssertionError(f"{sched.name}: {m.q.fin} of {sched.nframes} frames finished in {max_sweeps} sweeps")
    chk.finish(range(sched.nframes))
    return m, chk
