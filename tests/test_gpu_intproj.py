"""
GPU tests of bluest_intproj_eval (csrc/intproj.hip: k_intproj<NT>, the register-resident solve of csrc/solve.hpp in the one kernel
family that test_gpu_launch_matrix.py does not drive) at its own interface, in every instantiation NT, with N == NT and with the
most pads, against the 80-bit reference of tests/intproj_cases.py (whose soundness and coverage test_intproj_ref.py checks on the
CPU); and of the host search that feeds it (integer._search): chunking, the tie rules across chunk borders, and the selection
against an exhaustive evaluation of all 2^LL candidates by the reference.

Tolerances are those of intproj_cases.py (module docstring there): |V / V_ref - 1| <= tol_V per candidate, +inf exactly where
the reference has +inf.
"""
import ctypes

import numpy as np
import pytest

import intproj_cases as ic
from conftest import golden

pytestmark = pytest.mark.gpu

NTS = ic.nt_values()
GUARD, SENTINEL = 64, -7.25


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def _stream(torch):
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _raw(torch, N, n_out, LL, base, cols, ms):
    """one call of the entry point into a buffer with GUARD sentinels on each side; (rc, V (n_c, n_out) host, guards intact)"""
    from bluest_amd import _lib
    dev = torch.device("cuda", torch.cuda.current_device())
    b, c, m = (torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).to(dev) for x in (base, cols, ms))
    n_v = len(ms) * base.shape[0]
    buf = torch.full((2 * GUARD + n_v,), SENTINEL, dtype=torch.float64, device=dev)
    rc = _lib.lib().bluest_intproj_eval(N, n_out, LL, b.data_ptr(), c.data_ptr(), m.data_ptr(), len(ms), buf.data_ptr() + 8 * GUARD,
                                        _stream(torch))
    torch.cuda.synchronize()
    h = buf.cpu().numpy()
    intact = bool((h[:GUARD] == SENTINEL).all() and (h[GUARD + n_v:] == SENTINEL).all())
    return rc, h[GUARD:GUARD + n_v].reshape(len(ms), base.shape[0]), intact


def _library_call(torch, L):
    from bluest_amd import integer
    dev = torch.device("cuda", torch.cuda.current_device())
    V = integer.candidate_variances(L["N"], torch.from_numpy(L["base"]), L["cols"], L["ms"].T, dev)
    return V.cpu().numpy()


def _compare(V, refs, tag):
    """asserts of one launch; returns (worst error, its bound, worst error / bound) over the finite candidates, by class"""
    worst = {"well": (0.0, 0.0, 0.0), "ill": (0.0, 0.0, 0.0)}
    for c, row in enumerate(refs):
        for o, r in enumerate(row):
            if r["kind"] != ic.OK:
                assert V[c, o] == np.inf, tag + (c, o, r["kind"], V[c, o])          # not NaN, not a large number
                continue
            err = abs(V[c, o] / r["V"] - 1)
            key = "well" if r["cond"] <= ic.COND_WELL else "ill"
            if err / r["tol"] >= worst[key][2]:
                worst[key] = (err, r["tol"], err / r["tol"])
            assert err <= r["tol"], tag + (c, o, V[c, o], r["V"], err, r["tol"], r["cond"])
    return worst


@pytest.mark.parametrize("N", ic.table_n(NTS))
def test_kernel_against_ld_reference(gpu, N):
    """every launch of the table at this N through integer.candidate_variances: values, +inf, and the same bits twice"""
    nt = ic.nt_of(N, NTS)
    worst = {"well": (0.0, 0.0, 0.0), "ill": (0.0, 0.0, 0.0)}
    launches = ic.launches(N, NTS)
    assert {(L["LL"], L["n_out"]) for L in launches} == set(ic.settings(N, NTS))
    for L in launches:
        tag = (N, nt, L["LL"], L["n_out"], L["variant"])
        V = _library_call(gpu, L)
        assert V.shape == (len(L["ms"]), L["n_out"])
        w = _compare(V, ic.reference(L), tag)
        for k in w:
            if w[k][2] >= worst[k][2]:
                worst[k] = w[k]
        again = _library_call(gpu, L)
        assert V.tobytes() == again.tobytes(), tag
    print("intproj N = %d NT = %d: well-conditioned worst |V/Vref - 1| = %.2e (bound %.2e); ill-conditioned %.2e (bound %.2e)"
          % (N, nt, worst["well"][0], worst["well"][1], worst["ill"][0], worst["ill"][1]))


def test_many_candidates(gpu):
    """n_cand = 70000 > 65535: the candidate index (blockIdx.x, the offsets cand * LL and cand * n_out) beyond 16 bits; and 1"""
    L = ic.launch(8, 7, 1, "full")
    refs = ic.reference(L)
    rows = np.arange(7) % len(L["ms"])
    rows[5:] = [0, 1]
    ms7 = L["ms"][rows].copy()
    ms7[5:] += 1.0                                          # 7 distinct rows: the table's 5 and two more dense ones
    assert len({r.tobytes() for r in ms7}) == 7
    ref7 = [[ic.reference_one(8, L["base"][0], L["cols"][0], m)] for m in ms7]
    n_c = 70000
    reps = -(-n_c // 7)
    ms = np.tile(ms7, (reps, 1))[:n_c]
    rc, V, intact = _raw(gpu, 8, 1, 7, L["base"], L["cols"], ms)
    assert rc == 0 and intact
    _compare(V[:7], ref7, ("many",))
    assert [r[0]["kind"] for r in ref7[:5]] == [r[0]["kind"] for r in refs]
    want = np.tile(V[:7], (reps, 1))[:n_c]
    assert V.tobytes() == want.tobytes()                    # V[c] = V[c mod 7] bit for bit
    for c in range(7):
        rc, V1, intact = _raw(gpu, 8, 1, 7, L["base"], L["cols"], ms7[c:c + 1])
        assert rc == 0 and intact and V1.tobytes() == V[c:c + 1].tobytes()


def test_output_layout(gpu):
    """V[c, o] at cand * n_out + o with three different covariances; nothing written outside the n_cand * n_out doubles"""
    for N, LL in ((13, 7), (64, 1)):
        L = ic.launch(N, LL, 3, "full")
        refs = ic.reference(L)
        zero = L["kinds"].index("zero")
        assert len({refs[zero][o]["V"] for o in range(3)}) == 3      # the outputs differ
        rc, V, intact = _raw(gpu, N, 3, LL, L["base"], L["cols"], L["ms"])
        assert rc == 0 and intact
        assert not (V == SENTINEL).any()
        _compare(V, refs, ("layout", N))
        # one output at a time gives the same numbers: the output index only selects base and columns
        for o in range(3):
            rc, V1, intact = _raw(gpu, N, 1, LL, L["base"][o:o + 1], L["cols"][o:o + 1], L["ms"])
            assert rc == 0 and intact and V1[:, 0].tobytes() == np.ascontiguousarray(V[:, o]).tobytes()


BAD_CALLS = [("N_0", dict(N=0)), ("N_65", dict(N=65)), ("LL_0", dict(LL=0)), ("LL_33", dict(LL=33)), ("n_out_0", dict(n_out=0)),
             ("n_out_65536", dict(n_out=65536)), ("n_cand_0", dict(n_cand=0)), ("n_cand_2p31", dict(n_cand=1 << 31)),
             ("null_base", dict(base=None)), ("null_cols", dict(cols=None)), ("null_ms", dict(ms=None)), ("null_V", dict(V=None))]


@pytest.mark.parametrize("name,change", BAD_CALLS, ids=[n for n, _ in BAD_CALLS])
def test_argument_checks(gpu, name, change):
    """calls that the entry point rejects on the host before any launch: BluestHipError, V untouched; a valid call still works"""
    torch = gpu
    from bluest_amd import _lib
    dev = torch.device("cuda", torch.cuda.current_device())
    L = ic.launch(8, 7, 1, "full")
    n_c = len(L["ms"])
    t = {k: torch.from_numpy(L[k]).to(dev) for k in ("base", "cols", "ms")}
    t["V"] = torch.full((n_c,), SENTINEL, dtype=torch.float64, device=dev)
    a = dict(N=8, n_out=1, LL=7, n_cand=n_c)
    a.update({k: v.data_ptr() for k, v in t.items()})
    a.update(change)
    with pytest.raises(_lib.BluestHipError):
        _lib.check(_lib.lib().bluest_intproj_eval(a["N"], a["n_out"], a["LL"], a["base"], a["cols"], a["ms"], a["n_cand"], a["V"],
                                                  _stream(torch)))
    torch.cuda.synchronize()
    assert bool((t["V"] == SENTINEL).all())
    rc, V, intact = _raw(torch, 8, 1, 7, L["base"], L["cols"], L["ms"])
    assert rc == 0 and intact
    _compare(V, ic.reference(L), ("valid after " + name,))


# ---- the host search -------------------------------------------------------------------------------------------------------

class _Problem(object):
    def __init__(self, P):
        from bluest_amd import synth
        from bluest_amd.mosap import MOSAP
        from bluest_amd.sap import SAP
        self.P = P
        N = P["N"]
        costs = synth.group_costs(P["groups"], P["w"])
        if P["multi"]:
            Cs = [synth.wishart_covariance(N, o)[0] for o in range(P["n_out"])]
            mcosts = [synth.group_costs(mg, P["w"]) for mg in P["multi_groups"]]
            self.op = MOSAP(Cs, P["kmax"], [P["kmax"]] * P["n_out"], [g.tolist() for g in P["groups"]],
                            [[g.tolist() for g in mg] for mg in P["multi_groups"]], costs, mcosts, verbose=False)
            self.saps, self.mappings = self.op.SAPS, self.op.mappings
        else:
            self.op = SAP(synth.wishart_covariance(N, 0)[0], P["kmax"], [g.tolist() for g in P["groups"]], costs, verbose=False)
            self.saps, self.mappings = [self.op], [np.arange(self.op.L)]
        self.costs, self.e, self.plan = costs, self.op.e, self.op.plan

    def search(self, mode):
        from bluest_amd import integer
        P = self.P
        kw = dict(budget=P["budget"], eps=None) if mode == "budget" else dict(budget=None, eps=P["eps"])
        return integer._search(P["sol"], P["N"], self.costs, self.e, self.saps, self.mappings, self.plan, kw["budget"], kw["eps"],
                               ic.cap_rows(P), P["lb"], P["ub"], P["idx"], P["multi"])


@pytest.fixture(scope="module")
def problems(gpu):
    return [_Problem(ic.search_problem_single()), _Problem(ic.search_problem_ragged(golden("mosap_n6_o3_ragged.npz")))]


def test_search_is_independent_of_chunking(gpu, problems, monkeypatch):
    """chunks of 2^3 candidates against one chunk (the caps of the problems are applied per chunk): the same point and the same
    objective bits, in both modes; the exact tie of the
    single-output problem is decided as the reference decides it: budget mode by the LAST candidate (the copy at free entry 9),
    eps mode by the FIRST cheapest (the original at free entry 0)"""
    from bluest_amd import integer
    calls = []
    real = integer.candidate_variances

    def counting(*a, **k):
        calls.append(a[3].shape[1])
        return real(*a, **k)

    monkeypatch.setattr(integer, "candidate_variances", counting)
    default_bits = integer.CHUNK_BITS
    for pr in problems:
        P = pr.P
        LL = len(P["idx"])
        assert 8 <= LL <= 11 and default_bits >= LL
        for mode in ("budget", "eps"):
            del calls[:]
            val1, f1 = pr.search(mode)
            assert len(calls) == 1                                               # the default: one chunk
            monkeypatch.setattr(integer, "CHUNK_BITS", 3)
            del calls[:]
            val3, f3 = pr.search(mode)
            monkeypatch.setattr(integer, "CHUNK_BITS", default_bits)
            assert len(calls) > 8 and max(calls) <= 8                              # many chunks of at most 8 candidates
            assert val1 is not None and np.isfinite(f1)
            assert np.array_equal(val1, val3), (P["name"], mode)
            assert np.float64(f1).tobytes() == np.float64(f3).tobytes(), (P["name"], mode, f1, f3)
            if P["tie"] is not None:
                a, b = P["tie"]
                cols_equal = np.array_equal(integer.psi_column(pr.saps[0], int(P["idx"][a])), integer.psi_column(pr.saps[0], int(P["idx"][b])))
                assert cols_equal and pr.costs[P["idx"][a]] == pr.costs[P["idx"][b]]
                assert b >= 3                                                    # the two free entries meet across a chunk border
                got = (int(val1[P["idx"][a]]), int(val1[P["idx"][b]]))
                assert got == ((0, 1) if mode == "budget" else (1, 0)), (mode, got)


def test_search_against_exhaustive_reference(gpu, problems, monkeypatch):
    """all 2^LL candidates by the 80-bit reference from the base and the columns that _search itself hands to the kernel, the
    host's filters (model-0 coverage with in_out, budget * 1.0001, sample caps) restated here: the point returned passes them and
    is the best (budget) / the cheapest feasible one (eps)"""
    from bluest_amd import integer
    real = integer.candidate_variances
    seen = []

    def capturing(N, base_phi, cols, ms, device):
        seen.append((base_phi.cpu().numpy().copy(), np.array(cols), np.array(ms)))
        return real(N, base_phi, cols, ms, device)

    monkeypatch.setattr(integer, "candidate_variances", capturing)
    for pr in problems:
        P = pr.P
        N, idx, LL = P["N"], P["idx"], len(P["idx"])
        ms_all = ic.all_candidates(P)
        baseval = np.round(P["sol"]).astype(np.int64)
        baseval[idx] = 0
        cost = pr.costs @ baseval + ms_all @ pr.costs[idx]
        # model 0: some output that needs it gets a sample of a group with model 0 that the output has
        e = np.asarray(pr.e)
        covered = np.zeros(len(ms_all), dtype=bool)
        needs = 0
        for n, mp in enumerate(pr.mappings):
            if e[mp] @ baseval[mp] >= 1:
                continue
            needs += 1
            has = np.isin(idx, mp)
            covered |= ms_all @ (e[idx] * has) >= 1
        assert needs >= 1
        # caps: no model gets more samples than its cap, fixed and free entries together
        ES, rhs = ic.cap_rows(P)
        capped = np.ones(len(ms_all), dtype=bool)
        for ees, rr in zip(ES, rhs):
            assert ees @ baseval <= rr
            capped &= ees @ baseval + ms_all @ ees[idx] <= rr
        assert len(ES) >= 1 and 16 < (covered & capped).sum() < 0.6 * covered.sum()      # the caps remove a good part, not all
        allowed = covered & capped
        V_ref = tol = None
        for mode in ("budget", "eps"):
            del seen[:]
            val, fval = pr.search(mode)
            assert val is not None and len(seen) == 1
            base, cols, ms_sent = seen[0]
            if V_ref is None:
                V_ref, tol, cond = ic.reference_batch(N, base, cols, ms_all)
                tol = float(tol.max())
                assert tol <= ic.CAP
                # the library's group inverses are symmetric only up to rounding, and the kernel reads one triangle where the
                # reference reads the other: an input perturbation of relative size asym, cond(Phi) times that in V
                sq = [M.reshape(N, N) for M in list(base) + [c for co in cols for c in co]]
                asym = max(float(np.abs(M - M.T).max()) / max(float(np.abs(M).max()), 1e-300) for M in sq)
                tol_f = tol + 2.0 * cond * asym                                  # cond: the largest of the 2^LL candidates
                print("%s: tol %.2e asymmetry of the inputs %.2e" % (P["name"], tol, asym))
            chosen = val[idx].astype(np.float64)
            code = int(((chosen == P["ub"]).astype(np.int64) << np.arange(LL)).sum())
            assert np.array_equal(ms_all[code], chosen) and np.array_equal(np.delete(val, idx), np.delete(baseval, idx))
            assert covered[code] and capped[code]
            Vmax = V_ref.max(axis=1)
            if mode == "budget":
                limit = 1.0001 * P["budget"]
                assert np.abs(cost / limit - 1).min() > 1e-6                     # no cost near the limit
                ok = allowed & (cost <= limit)
                assert ms_sent.shape[1] == ok.sum() and ok[code] and 16 < ok.sum() < len(ok) - 16
                assert np.isfinite(Vmax[ok]).any()
                best = Vmax[ok].min()
                uncapped = covered & (cost <= limit)
                assert not capped[uncapped & (Vmax == Vmax[uncapped].min())].any()    # the caps exclude the best point without them
                assert Vmax[code] <= best * (1 + 2 * tol), (P["name"], Vmax[code], best)
                assert abs(fval / Vmax[code] - 1) <= tol_f
                if P["tie"] is not None:                                         # the tie is live: two best candidates, the copies swapped
                    a, b = P["tie"]
                    winners = np.flatnonzero(ok & (Vmax == best))
                    assert len(winners) == 2 and winners[1] - winners[0] == (1 << b) - (1 << a) and code == winners[1]
            else:
                lim = 1.0001 * np.asarray(P["eps"]) ** 2
                rel = V_ref / lim[None, :]
                assert np.abs(rel - 1).min() > 1e-6 > tol                        # no candidate inside the margins
                assert ms_sent.shape[1] == allowed.sum()
                feasible = allowed & np.all(V_ref <= lim[None, :] * (1 + tol / 1.0001), axis=1)
                strict = allowed & np.all(V_ref <= lim[None, :] * (1 - tol / 1.0001), axis=1)
                assert np.array_equal(feasible, strict) and 8 <= strict.sum() < allowed.sum() - 16
                assert feasible[code]
                assert cost[code] <= cost[strict].min()
                assert abs(fval / Vmax[code] - 1) <= tol_f
                if P["tie"] is not None:
                    a, b = P["tie"]
                    cheapest = np.flatnonzero(strict & (cost == cost[strict].min()))
                    assert len(cheapest) == 2 and cheapest[1] - cheapest[0] == (1 << b) - (1 << a) and code == cheapest[0]
