"""The refill schedules of tests/test_gpu_mf_refill.py through the numpy model alone (no GPU): every schedule keeps
the checker's invariants I1 .. I5 and reaches the path it is named for, so the GPU replay of the same schedule
exercises that path whatever the host's timing."""
import numpy as np
import pytest
from mf_refill_model import (MAX_ITER, SRC_COLD, SRC_HOSTX0, SRC_LAST, SRC_NONE, SRC_SLOT, SUCCESS, cases, replay,
                             schedules)


# schedules that fill more than 64 slots at 128 frames (both words of the plan's ballots)
BOTH_WORDS = ("steady", "ring_pressure", "max_iter", "knobs_capq_age0", "knobs_nochain_x0", "knobs_nochain_cold")


def _kinds(m):
    return [k for pl in m.plans for k in pl.kinds]


def _final_log(m, nframes):
    """frame -> (status, iters, flags, warm_from, warm_live, warm_iter) from the ring log (rings that hold the whole series)."""
    L = m.log
    return {int(L.frame[i]): (int(L.status[i]), int(L.iters[i]), int(L.flags[i]), int(L.warm_from[i]),
                              int(L.warm_live[i]), int(L.warm_iter[i])) for i in range(min(nframes, m.p.rcap))}


def check_path(name, m, sched, nf):
    P, kinds = m.plans, _kinds(m)
    n = sched.nframes
    assert m.q.fin == n and m.q.q_head == n
    if nf == 128 and name in BOTH_WORDS:
        assert any(pl.words[0] and pl.words[1] for pl in P), "admissions in both ballot words"
        assert any(pl.ret_words[1] for pl in P), "retirements in the second ballot word"
    if name == "steady":
        assert sum(pl.idle for pl in P) == 1 and any(pl.src_live for pl in P if pl.n_adm)
        assert kinds.count(SRC_NONE) == nf and set(kinds) == {SRC_NONE, SRC_SLOT}
    elif name == "lagging":
        assert sum(1 for pl in P if pl.n_adm and not pl.idle) >= 4  # admissions spread over the sweeps
    elif name == "starved":
        assert any(pl.idle and pl.n_adm == 0 and pl.n_ret == 0 for pl in P[1:]), "an idle plan with nothing to do"
        hits = [pl for pl in P if pl.idle and pl.n_adm and set(pl.kinds) == {SRC_LAST}]
        assert len(hits) >= 3 and any(pl.n_adm > 1 for pl in hits), "all_done = 1 plans admitting from xlast"
        assert all(pl.src_live == 0 for pl in P if pl.n_adm)
    elif name == "ring_pressure":
        assert any(pl.waiting > 1 for pl in P), "finished frames waiting for ring room"
        assert any(pl.src_waiting and pl.n_adm for pl in P), "a waiting finished frame as the source"
        assert any(pl.idle and pl.n_ret for pl in P), "a retirement by a plan that ran alone"
    elif name == "queue_wrap":
        assert n > 3 * m.p.qcap and m.q.q_head > 3 * m.p.qcap
    elif name == "nonfinite":
        log = _final_log(m, n)
        assert log[0][1:3] == (0, 1) and log[nf + 1][1:3] == (0, 1)  # NaN at own sweep 0: no rollback
        assert log[2][1:3] == (2, 3) and log[nf + 3][1:3] == (1, 3)  # later: rolled back to Xprev
        assert sum(pl.ret_prev for pl in P) == 2
        for v in log.values():  # never a source once non-finite (before that: in flight, like any frame)
            assert v[3] not in sched.nan_at or (v[4] == 1 and v[5] <= sched.nan_at[v[3]]), v
        assert sum(pl.n_adm for pl in P) == n  # the slots refilled
    elif name == "max_iter":
        log = _final_log(m, n)
        assert any(v[0] == MAX_ITER and v[1] == m.p.max_iter for v in log.values())
        assert any(v[0] == SUCCESS for v in log.values())
        assert any(pl.skip_bwd and pl.nmax for pl in P), "a sweep whose running slots are all at max_iter"
    elif name == "knobs_cap1_age3":
        assert all(pl.n_adm <= 1 for pl in P) and SRC_SLOT in kinds
    elif name == "knobs_capq_age0":
        assert max(pl.n_adm for pl in P) == max(1, nf // 4) and any(pl.src_live for pl in P if pl.n_adm)
    elif name == "knobs_src_finished":
        assert all(not pl.src_live for pl in P) and {SRC_SLOT, SRC_LAST} & set(kinds)
    elif name == "knobs_lead":
        assert P[0].kinds == [SRC_COLD] and kinds.count(SRC_COLD) == 1
        first = next(i for i, pl in enumerate(P) if i and pl.n_adm)
        assert all(pl.n_adm == 0 for pl in P[1:first]) and P[first].n_ret == 1  # alone until it has finished
    elif name == "knobs_nochain_x0":
        assert kinds[:nf] == [SRC_HOSTX0] * nf and set(kinds[nf:]) == {SRC_COLD}
    elif name == "knobs_nochain_cold":
        assert set(kinds) == {SRC_COLD}
    elif name == "knobs_chain_x0":
        assert SRC_HOSTX0 in kinds and SRC_SLOT in kinds and kinds[0] == SRC_HOSTX0
    elif name == "knobs_extrap4":
        assert any(pl.src_live and pl.n_adm for pl in P)
    elif name == "knobs_drift1":
        assert sum(pl.xlast_moved for pl in P) >= 3 and m.drift_uses >= 3
    else:
        raise AssertionError(f"no path assertion for schedule {name}")


@pytest.mark.parametrize("name,nf,log", cases())
def test_schedule_reaches_its_path(name, nf, log):
    sched = schedules(nf)[name]
    m, chk = replay(sched, nf, log)  # (replay feeds the checker after every sweep and closes I1 at the end)
    check_path(name, m, sched, nf)
    if sched.kw.get("src_extrap") or sched.kw.get("src_age"):
        assert chk.ever_live


def test_stage_model_matches_fp64_formulas():
    """The staging model against the formulas it stands for (max, sum of squares over positive pixels)."""
    from mf_refill_model import RefillModel, params, pixels
    p = params(nf=16, nframes=4)
    m = RefillModel(p)
    g = pixels(np.random.default_rng(1), 4, p.nrows)
    m.g64q[:4, :p.nrows] = g
    stats = m.stage_stats(0, 4)
    m.stage_norm(stats, 0, 10, True, 4)
    for j in range(4):
        v = np.where(np.isfinite(g[j]), g[j], -1.0)
        assert stats[j] == v.max()
        np.testing.assert_allclose(stats[16 + j], np.sum(v[v > 0] ** 2), rtol=1e-14)
        np.testing.assert_allclose(m.q.q_G[j], np.sum((v[v > 0] / v.max()) ** 2), rtol=1e-14)
        assert m.q.q_frame[j] == 10 + j and m.q.q_cold[j] == 1 and m.q.q_norm[j] == v.max()
        assert np.array_equal(m.ghq[j, :p.nrows], (v / v.max()).astype(np.float32)) and not m.ghq[j, p.nrows:].any()
