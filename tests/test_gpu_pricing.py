"""
GPU tests of the three small kernels around the Newton master of the second-order finish (csrc/newton.hip: k_price,
k_support_point, k_ma_update) at their own interface, against the plain restatement oracle/pricing_ref.py on the case table
tests/pricing_cases.py (whose coverage test_pricing_ref.py checks on the CPU).  The master kernel itself is not called here.

bluest_price / bluest_price_capped: c_sup, all 1024 (top_val, top_idx) pairs and y0 bit-equal to the reference -- the kernel's
arithmetic is explicit fmas, one product and one sum, each correctly rounded on both sides, and everything else is discrete.
bluest_support_point: bit-equal to one of the two roundings the compiler's default contraction allows, the same one for all i.
bluest_ma_update: bit-equal for one output and for p = 1 (no pow); for p = 32 within pricing_cases.ma_bound.

Every call hands over buffers of at least their documented size, support indices in [0, L) ascending, cap masks without bits
at or above the number of caps; every output buffer carries poisoned padding that must come back untouched.
"""
import ctypes

import numpy as np
import pytest

import pricing_cases as pc
from oracle import pricing_ref as ref

pytestmark = pytest.mark.gpu

PAD, POISON_F, POISON_I = 8, -7.25e77, -77
PRICE_CASES = pc.all_price_cases()
_plans, _hip = {}, []


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("these tests need the GPU (run with -m gpu on the MI355X box)")
    return torch


def _peek(torch, address, n):
    """n doubles at a device address, through the HIP runtime the process already has loaded"""
    if not _hip:
        path = next(line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line)
        _hip.append(ctypes.CDLL(path))
        _hip[0].hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
        _hip[0].hipMemcpy.restype = ctypes.c_int
    torch.cuda.synchronize()
    out = np.empty(n, dtype=np.float64)
    assert _hip[0].hipMemcpy(out.ctypes.data, address, 8 * n, 2) == 0          # hipMemcpyDeviceToHost
    return out


def _plan(torch, sh, evaluate=True):
    """the shape's plan (built once), after one plan.eval: dict plan, grad (device, the evaluation's), v (host copy of the v
    workspace), var, status"""
    from bluest_amd._lib import check
    from bluest_amd.plan import Plan
    if sh["name"] not in _plans:
        plan = Plan(sh["n"], sh["L"], sh["outs"])
        assert plan.identity == (not sh["ragged"]) and plan.n_out == sh["n_out"] and plan.L == sh["L"]
        for o in range(sh["n_out"]):                                # the layout the synthetic gradients are packed for
            assert 0 <= plan.grad_off[o] and plan.grad_off[o] + sh["lens"][o] <= plan.grad_len
        _plans[sh["name"]] = dict(plan=plan)
    rec = _plans[sh["name"]]
    if evaluate and "v" not in rec:
        plan = rec["plan"]
        m = 0.5 + np.random.RandomState(sh["L"]).rand(sh["L"])
        var, grad, status = plan.eval(m)
        v = ctypes.c_void_p()
        check(plan.lib.bluest_plan_v_workspace(plan._h, ctypes.byref(v), None))
        rec.update(grad=grad, var=var.cpu().numpy()[0], status=status.cpu().numpy()[0], v=_peek(torch, v.value, sh["n_out"] * sh["n"]))
        assert (rec["status"] == 0).all()
    return _plans[sh["name"]]


def _up(torch, plan, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(plan.device)


def _padded(torch, plan, n, dtype=np.float64):
    return _up(torch, plan, np.full(n + PAD, POISON_I if dtype == np.int64 else POISON_F, dtype=dtype))


def _price(torch, plan, a, grad_dev=None, S=None):
    """one bluest_price / bluest_price_capped call; returns the four outputs (host) after checking their padding"""
    from bluest_amd._lib import check
    from bluest_amd.plan import _stream
    sup = a["sup"]
    S = len(sup) if S is None else S
    assert (np.diff(sup) > 0).all() and sup[0] >= 0 and sup[-1] < plan.L and len(a["cc"]) == plan.L and len(a["mu"]) == plan.n_out
    d = {k: _up(torch, plan, a[k]) for k in ("mu", "s", "cc", "sup")}
    grad = _up(torch, plan, a["grad"]) if grad_dev is None else grad_dev
    assert grad.numel() >= plan.grad_len
    c_sup, top_val, y0 = _padded(torch, plan, len(sup)), _padded(torch, plan, ref.PRICE_CANDIDATES), _padded(torch, plan, plan.n_out)
    top_idx = _padded(torch, plan, ref.PRICE_CANDIDATES, np.int64)
    with torch.cuda.device(plan.device):
        if a["capmask"] is not None:
            assert len(a["capmask"]) == plan.L and len(a["nu"]) == 64 and len(a["master_out"]) == 16 + plan.n_out
            cm, nu, mo = _up(torch, plan, a["capmask"].view(np.int64)), _up(torch, plan, a["nu"]), _up(torch, plan, a["master_out"])
            check(plan.lib.bluest_price_capped(plan._h, grad.data_ptr(), d["mu"].data_ptr(), d["s"].data_ptr(), d["cc"].data_ptr(), S,
                                               d["sup"].data_ptr(), c_sup.data_ptr(), top_val.data_ptr(), top_idx.data_ptr(), y0.data_ptr(),
                                               cm.data_ptr(), nu.data_ptr(), mo.data_ptr(), _stream()))
        else:
            check(plan.lib.bluest_price(plan._h, grad.data_ptr(), d["mu"].data_ptr(), d["s"].data_ptr(), d["cc"].data_ptr(), S,
                                        d["sup"].data_ptr(), c_sup.data_ptr(), top_val.data_ptr(), top_idx.data_ptr(), y0.data_ptr(), _stream()))
    torch.cuda.synchronize()
    out = {}
    for k, t, n in (("c_sup", c_sup, S), ("top_val", top_val, ref.PRICE_CANDIDATES), ("top_idx", top_idx, ref.PRICE_CANDIDATES), ("y0", y0, plan.n_out)):
        h = t.cpu().numpy()
        assert (h[n:] == (POISON_I if k == "top_idx" else POISON_F)).all(), "%s: written past its %d entries" % (k, n)
        out[k] = h[:n]
    return out


def _bits(x):
    return np.ascontiguousarray(x).view(np.int64)


def _compare_price(got, want, v):
    for k in ("top_idx", "top_val", "c_sup", "y0"):
        bad = np.flatnonzero(_bits(got[k]) != _bits(want[k]))
        assert bad.size == 0, "%s differs at %s: %r, reference %r" % (k, bad[:5], got[k][bad[:5]], want[k][bad[:5]])
    n_out = len(got["y0"])
    assert np.array_equal(_bits(got["y0"]), _bits(v[::len(v) // n_out]))         # entry o N of the v workspace
    # what the certified bound takes from the kernel: the first entry of every workgroup
    first_v, first_i = got["top_val"][::ref.PRICE_TOP], got["top_idx"][::ref.PRICE_TOP]
    cmax = want["c"].max()
    assert first_v.max().view(np.int64) == cmax.view(np.int64)
    assert first_i[first_v == first_v.max()].min() == int(np.flatnonzero(want["c"] == cmax)[0])


@pytest.mark.parametrize("name", [c["name"] for c in PRICE_CASES])
def test_price_synthetic(gpu, name):
    """planted maxima and ties, 0 / 3 / 64 caps, mu = 0 on an infinite gradient: every output bit-equal"""
    c = next(c for c in PRICE_CASES if c["name"] == name)
    rec = _plan(gpu, c["sh"])
    plan = rec["plan"]
    a = pc.inputs(c, plan.grad_off, plan.grad_len)
    a["v_ws"] = rec["v"]                                            # the kernel reads the plan's own workspace
    want = pc.reference(c, a)
    _compare_price(_price(gpu, plan, a), want, rec["v"])


@pytest.mark.parametrize("key,n_out,ragged", pc.PRICE_SHAPES, ids=[pc.shape(*s)["name"] for s in pc.PRICE_SHAPES])
def test_price_the_plans_own_gradient(gpu, key, n_out, ragged):
    """the gradient plan.eval left on the device, priced in place; the reference reads the host copy of the same buffer"""
    sh = pc.shape(key, n_out, ragged)
    rec = _plan(gpu, sh)
    plan = rec["plan"]
    a = pc.inputs(dict(sh=sh, patches=[], caps=0, inf=False), plan.grad_off, plan.grad_len)
    a["grad"], a["v_ws"] = rec["grad"].cpu().numpy()[0], rec["v"]
    sup = a["sup"]
    want = ref.price(sh["L"], n_out, a["grad"], a["goff"], sh["invmap"], a["mu"], a["s"], a["cc"], len(sup), sup, a["v_ws"], sh["n"])
    assert (want["c"] >= 0).all() and want["c"].max() > 0
    _compare_price(_price(gpu, plan, a, grad_dev=rec["grad"]), want, rec["v"])
    for o in range(n_out):                                          # y0 is V_o: row 0 of the inverse information matrix
        assert abs(rec["v"][o * sh["n"]] / rec["var"][o] - 1.0) < 1e-9


@pytest.mark.parametrize("name", [s[0] for s in pc.support_cases()])
def test_support_point(gpu, name):
    from bluest_amd import _lib
    torch = gpu
    _, L, S, sup, xs, cc, eps = next(s for s in pc.support_cases() if s[0] == name)
    assert len(sup) == S and (np.diff(sup) > 0).all() and sup[0] >= 0 and sup[-1] < L and len(cc) == L
    dev = torch.device("cuda", torch.cuda.current_device())
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)      # noqa: E731
    m = up(np.full(L + PAD, POISON_F))
    sup_d, xs_d, cc_d = up(sup), up(xs), up(cc)
    _lib.check(_lib.lib().bluest_support_point(L, S, sup_d.data_ptr(), xs_d.data_ptr(), cc_d.data_ptr(), float(eps), m.data_ptr(),
                                               ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    h = m.cpu().numpy()
    assert (h[L:] == POISON_F).all()
    sep, fused = ref.support_point(L, S, sup, xs, cc, eps)
    is_sep, is_fused = np.array_equal(_bits(h[:L]), _bits(sep)), np.array_equal(_bits(h[:L]), _bits(fused))
    print("%s: separate multiply-add %s, fma %s" % (name, is_sep, is_fused))
    assert is_sep or is_fused, (np.flatnonzero(h[:L] != sep)[:5], np.flatnonzero(h[:L] != fused)[:5])


def _ma(torch, plan, a):
    from bluest_amd._lib import check
    from bluest_amd.plan import _stream
    L, n_out = plan.L, plan.n_out
    assert len(a["var"]) == n_out and len(a["status"]) == n_out and len(a["grad"]) >= plan.grad_len and len(a["cc"]) == L and len(a["s"]) == n_out
    d = {k: _up(torch, plan, a[k]) for k in ("var", "status", "grad", "s", "cc")}
    x = _up(torch, plan, np.concatenate([a["x"], np.full(PAD, POISON_F)]))
    m = _up(torch, plan, np.concatenate([a["m"], np.full(PAD, POISON_F)]))
    with torch.cuda.device(plan.device):
        check(plan.lib.bluest_ma_update(plan._h, d["var"].data_ptr(), d["status"].data_ptr(), d["grad"].data_ptr(), d["s"].data_ptr(),
                                        d["cc"].data_ptr(), a["p"], x.data_ptr(), m.data_ptr(), _stream()))
    torch.cuda.synchronize()
    xh, mh = x.cpu().numpy(), m.cpu().numpy()
    assert (xh[L:] == POISON_F).all() and (mh[L:] == POISON_F).all()
    return xh[:L], mh[:L]


@pytest.mark.parametrize("key,n_out,ragged", pc.MA_SHAPES, ids=[pc.shape(*s)["name"] for s in pc.MA_SHAPES])
def test_ma_update(gpu, key, n_out, ragged):
    """p = 1 (and one output) bit-equal; p = 32 within ma_bound(n_out) relative, the largest error printed; a status not OK, an
    infinite and a zero r_max leave x and m bitwise alone"""
    sh = pc.shape(key, n_out, ragged)
    plan = _plan(gpu, sh, evaluate=False)["plan"]
    for p in (1.0, 32.0):
        a = pc.ma_inputs(sh, p, plan.grad_off, plan.grad_len)
        xr, mr, facts = pc.ma_reference(sh, a)
        assert facts["ok"]
        x, m = _ma(gpu, plan, a)
        if p == 1.0 or n_out == 1:
            assert np.array_equal(_bits(x), _bits(xr)) and np.array_equal(_bits(m), _bits(mr))
        else:
            nz = xr != 0.0                                          # (a group of no output: num = 0 on both sides)
            assert np.array_equal(x[~nz], xr[~nz]) and np.array_equal(m[~nz], mr[~nz])
            err = max(float(np.abs(x[nz] / xr[nz] - 1.0).max()), float(np.abs(m[nz] / mr[nz] - 1.0).max()))
            print("%s p=32: largest relative error %.3g = %.2f eps, bound %.0f eps" % (sh["name"], err, err / ref.DBL_EPS,
                                                                                 pc.ma_bound(n_out) / ref.DBL_EPS))
            assert err <= pc.ma_bound(n_out)
    for fault in ("status", "inf", "zero"):
        a = pc.ma_inputs(sh, 32.0, plan.grad_off, plan.grad_len, fault=fault)
        x, m = _ma(gpu, plan, a)
        assert np.array_equal(_bits(x), _bits(a["x"])) and np.array_equal(_bits(m), _bits(a["m"])), fault


def test_ma_update_refuses_65_outputs(gpu):
    from bluest_amd import _lib
    sh = pc.shape("n4", 65, False)
    plan = _plan(gpu, sh, evaluate=False)["plan"]
    a = pc.ma_inputs(sh, 32.0, plan.grad_off, plan.grad_len)
    with pytest.raises(_lib.BluestHipError, match="error 1.*64 outputs"):
        _ma(gpu, plan, a)


def test_argument_checks(gpu):
    """what the host refuses before any launch: null pointers, an unfinalized plan, L <= 0, S <= 0 (bluest_price* too); a valid
    call still succeeds afterwards"""
    from bluest_amd import _lib
    torch = gpu
    L_ = _lib.lib()
    sh = pc.shape("n6", 3, True)
    rec = _plan(torch, sh)
    plan = rec["plan"]
    c = next(c for c in PRICE_CASES if c["name"] == sh["name"] + "-caps3")
    a = pc.inputs(c, plan.grad_off, plan.grad_len)
    a["v_ws"] = rec["v"]
    names = ("grad", "mu", "s", "cc", "sup", "c_sup", "top_val", "top_idx", "y0", "capmask", "nu", "master_out")
    host = dict(a, capmask=a["capmask"].view(np.int64), c_sup=np.zeros(len(a["sup"])), top_val=np.zeros(ref.PRICE_CANDIDATES),
                top_idx=np.zeros(ref.PRICE_CANDIDATES, dtype=np.int64), y0=np.zeros(3))
    d = {k: _up(torch, plan, host[k]) for k in names}
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    S = len(a["sup"])

    def price(handle=plan._h, S=S, capped=True, **null):
        p = [None if k in null else d[k].data_ptr() for k in names]
        if capped:
            return L_.bluest_price_capped(handle, *p[:4], S, *p[4:], st)
        return L_.bluest_price(handle, *p[:4], S, *p[4:9], st)
    with torch.cuda.device(plan.device):
        assert price() == 0 and price(capped=False) == 0
        for k in names[:9]:
            assert price(**{k: 1}) == ref.ERR_ARG and price(capped=False, **{k: 1}) == ref.ERR_ARG, k
        assert price(nu=1) == ref.ERR_ARG and price(master_out=1) == ref.ERR_ARG
        assert price(handle=None) == ref.ERR_ARG and price(handle=None, capped=False) == ref.ERR_ARG
        for bad in (0, -1, -(2 ** 31)):
            assert price(S=bad) == ref.ERR_ARG and price(S=bad, capped=False) == ref.ERR_ARG, bad
        raw = ctypes.c_void_p()
        _lib.check(L_.bluest_plan_create(ctypes.byref(raw), sh["n"], sh["L"]))
        try:
            assert price(handle=raw) == ref.ERR_STATE and price(handle=raw, capped=False) == ref.ERR_STATE
            ma = [d[k].data_ptr() for k in ("mu", "sup", "grad", "s", "cc")]
            assert L_.bluest_ma_update(raw, *ma, 32.0, d["c_sup"].data_ptr(), d["top_val"].data_ptr(), st) == ref.ERR_STATE
        finally:
            L_.bluest_plan_destroy(raw)
        # bluest_ma_update: var, status, grad, s, cc, x, m
        b = pc.ma_inputs(sh, 32.0, plan.grad_off, plan.grad_len)
        md = [_up(torch, plan, b[k]) for k in ("var", "status", "grad", "s", "cc", "x", "m")]
        for k in range(7):
            p = [None if j == k else t.data_ptr() for j, t in enumerate(md)]
            assert L_.bluest_ma_update(plan._h, *p[:5], 32.0, *p[5:], st) == ref.ERR_ARG
        assert L_.bluest_ma_update(None, *[t.data_ptr() for t in md[:5]], 32.0, md[5].data_ptr(), md[6].data_ptr(), st) == ref.ERR_ARG
        # bluest_support_point: sup, xs, cc, m
        xs = _up(torch, plan, np.full(S, 1.0 / S))
        m = _up(torch, plan, np.zeros(sh["L"]))
        sp = [d["sup"].data_ptr(), xs.data_ptr(), d["cc"].data_ptr()]
        for k in range(4):
            p = [None if j == k else v for j, v in enumerate(sp + [m.data_ptr()])]
            assert L_.bluest_support_point(sh["L"], S, *p[:3], 1e-3, p[3], st) == ref.ERR_ARG
        for Lbad, Sbad in ((0, S), (-1, S), (sh["L"], 0), (sh["L"], -1)):
            assert L_.bluest_support_point(Lbad, Sbad, *sp, 1e-3, m.data_ptr(), st) == ref.ERR_ARG
        assert L_.bluest_support_point(sh["L"], S, *sp, 1e-3, m.data_ptr(), st) == 0
    torch.cuda.synchronize()
    _compare_price(_price(torch, plan, a), pc.reference(c, a), rec["v"])
