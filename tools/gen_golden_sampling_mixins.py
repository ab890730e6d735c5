"""
Write tests/golden/sampling_mixins.npz: the bits of everything the sampling and pilot mix-ins return on the toy problems of the host
tests, with the numpy restatements of tests/ standing in for the GPU wrappers (no GPU is needed):

    python tools/gen_golden_sampling_mixins.py

The file is a record of the commit it was written at.  tests/test_sampling_mixins_bits.py calls record() again and compares every
array bit for bit, so a change to the Python of the mix-ins that moves a bit, a sampler call or a flush shows.  Regenerate it only
for a change that is meant to move them.

What is recorded (keys "<problem>/<flush>/<what>"; flush = "default" or "each", a flush after every group):
  scalar_<case>   MomentsMixin over tests/golden/estimator_case_<case>.npz: solve(), variance_test(N=3), sampled_errors of both
                  sources, pooled_covariances(), sample_moments, the sampler calls
  field_plain, field_stream0, field_stream13440, field_cov
                  the field problem of tests/test_field_stream_host.py under FieldErrorsMixin, with StreamedFieldsMixin at the
                  thresholds 0 and 13440, and with FieldCovariancesMixin in front of FieldErrorsMixin: the same, and
                  sampled_error_fields(), field_sample_moments, field_sample_covariances
  pilot_<...>, field_pilot_<...>
                  both pilot mix-ins on the seeded problems of their host tests without a tolerance, with one, and capped: the
                  errors, C and dV, pilot_report, what was printed, the sampler calls
  unpacked_*      the two triangle unpackers on random packed data
Sampler calls are rows [N, len(ls), ls padded with -1]; a report is [samples, rounds, ratio, converged, capped_by] with NaN for
None and capped_by 0 = None, 1 = "samples", 2 = "bytes", -1 = no such key.
"""
import contextlib
import io
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for path in (os.path.join(ROOT, "tests"), ROOT):
    if path not in sys.path:
        sys.path.insert(0, path)
OUT = os.path.join(ROOT, "tests", "golden", "sampling_mixins.npz")
EPS = [0.2, 0.3]


@contextlib.contextmanager
def patched(*settings):
    """with patched((module, name, value), ...): the attributes are set inside and put back afterwards"""
    before = [(m, k, getattr(m, k)) for m, k, _ in settings]
    try:
        for m, k, v in settings:
            setattr(m, k, v)
        yield
    finally:
        for m, k, v in before:
            setattr(m, k, v)


def restatements():
    """every GPU wrapper the mix-ins call -> its numpy restatement, at the module attribute the mix-ins look it up in"""
    import field_accum_ref
    import field_cov_ref
    import field_moments_ref
    import field_pilot_ref
    import fields_ref
    import gsums_ref
    import moments_ref
    import pilot4_ref
    import pilot_ref
    from bluest_amd import (estimator, field_covariances, field_errors, field_pilot_errors, field_stream, fields, moments, pilot,
                            pilot_errors)
    return patched(
        (estimator, "group_sums", lambda values, weights=None, repeat_of=None, R=None, slab_bytes=None:
            gsums_ref.group_sums(values, weights, repeat_of, R)),
        (moments, "group_moments", lambda values, slab_bytes=None: moments_ref.group_moments(values)),
        (fields, "field_group_sums", lambda values, **kw: fields_ref.field_group_sums(values, **kw)),
        (fields, "field_statistics", lambda values, w, differences=True: fields_ref.field_statistics(values, w, differences)),
        (field_errors, "field_weighted_moments", lambda values, coef, **kw: field_moments_ref.field_weighted_moments(values, coef)),
        (field_covariances, "field_group_moments", lambda values, w, with_first=False, slab_bytes=None:
            field_cov_ref.field_group_moments(values, w, with_first=with_first)),
        (field_stream, "FieldAccumulator", field_accum_ref.StubAccumulator),
        (pilot, "pilot_statistics", lambda values, differences=True: pilot_ref.pilot_statistics(values, differences)),
        (pilot_errors, "pilot_fourth_moments", lambda values, differences=True, shift=None, slab_bytes=None:
            pilot4_ref.pilot_fourth_moments(values, differences, shift)),
        (field_pilot_errors, "field_pilot_moments", lambda values, w, centre=None, differences=True, **kw:
            field_pilot_ref.field_pilot_moments(values, w, centre, differences)))


def flush_sizes(which):
    from bluest_amd import estimator, fields
    if which == "default":
        return patched()
    return patched((estimator, "SLAB_BYTES", 1), (fields, "SLAB_BYTES", 1))


def calls_array(calls, width=3):
    rows = np.full((len(calls), 2 + width), -1, dtype=np.int64)
    for row, (ls, N) in zip(rows, calls):
        row[0], row[1], row[2:2 + len(ls)] = N, len(ls), ls
    return rows


def report_array(report):
    none = lambda x: np.nan if x is None else float(x)
    capped = {None: 0.0, "samples": 1.0, "bytes": 2.0}[report["capped_by"]] if "capped_by" in report else -1.0
    assert sorted(set(report) - {"capped_by"}) == ["converged", "ratio", "rounds", "samples"]
    return np.array([none(report["samples"]), none(report["rounds"]), none(report["ratio"]), none(report["converged"]), capped])


def put(got, prefix, **arrays):
    for key, value in arrays.items():
        value = np.asarray(value)
        got["%s/%s" % (prefix, key)] = value if value.dtype.kind in "iu" else np.ascontiguousarray(value, dtype=np.float64)


# ---- the scalar problem: MomentsMixin over the estimator fixtures ------------------------------------------------------------------
def scalar(got, name, flush):
    import gsums_ref
    from bluest_amd.blue_models import BLUEProblem
    from bluest_amd.estimator import SamplingMixin
    from bluest_amd.moments import MomentsMixin
    from test_estimator_host import hand_set
    g = gsums_ref.case(name)
    K, eps, n_calls = int(g["K"]), float(g["eps"]), int(g["solve_calls"])
    p = gsums_ref.replay_class(g, MomentsMixin, SamplingMixin, BLUEProblem)()
    hand_set(p, g)
    prefix = "scalar_%s/%s" % (name, flush)
    mus, errs, cost = p.solve(K=K, eps=eps)
    put(got, prefix, mus=mus, errs=errs, cost=[cost], sampled=p.sampled_errors("samples"), model=p.sampled_errors("model"),
        groups=sorted(p.sample_moments), solve_calls=calls_array(p.calls, int(g["M"])))
    for gi, (N, C) in p.sample_moments.items():
        put(got, prefix, **{"N_%d" % gi: [N], "C_%d" % gi: C})
    Cs, dofs = p.pooled_covariances()
    put(got, prefix, pooled=Cs, dof=dofs)
    p.start, p.calls = n_calls, []
    ex, err = p.variance_test(eps=eps, K=K, N=3)
    put(got, prefix, vt_ex=ex, vt=err, vt_calls=calls_array(p.calls, int(g["M"])))


# ---- the field problem of tests/test_field_stream_host.py ----------------------------------------------------------------------------
def field(got, name, flush):
    from bluest_amd.blue_models import BLUEProblem
    from bluest_amd.estimator import SamplingMixin
    from bluest_amd.field_covariances import FieldCovariancesMixin
    from bluest_amd.field_errors import FieldErrorsMixin
    from bluest_amd.field_stream import StreamedFieldsMixin
    from bluest_amd.fields import FieldOutputsMixin
    from test_field_stream_host import hand_set, toy
    base = (FieldErrorsMixin, FieldOutputsMixin, SamplingMixin, BLUEProblem)
    bases, kw = {"plain": (base, {}),
                 "stream0": ((StreamedFieldsMixin,) + base, dict(field_stream_bytes=0)),
                 "stream13440": ((StreamedFieldsMixin,) + base, dict(field_stream_bytes=13440)),
                 "cov": ((FieldCovariancesMixin,) + base, {})}[name]
    p = toy(bases, **kw)
    hand_set(p)
    prefix = "field_%s/%s" % (name, flush)
    mus, errs, cost = p.solve(K=3, eps=EPS)
    maps, unsampled = p.sampled_error_fields()
    put(got, prefix, mus0=[mus[0]], mus1=mus[1], errs=errs, cost=[cost], sampled=p.sampled_errors("samples"),
        model=p.sampled_errors("model"), map0=[maps[0]], map1=maps[1], unsampled=unsampled,
        field_errors_sampled=FieldErrorsMixin.sampled_errors(p, "samples"), solve_calls=calls_array(p.calls))
    for n, per_group in enumerate(p.field_sample_moments):
        put(got, prefix, **{"groups_%d" % n: sorted(per_group)})
        for gi, (N, var) in per_group.items():
            put(got, prefix, **{"N_%d_%d" % (n, gi): [N], "var_%d_%d" % (n, gi): var})
    if name == "cov":
        for n, per_group in enumerate(p.field_sample_covariances):
            put(got, prefix, **{"cov_groups_%d" % n: sorted(per_group)})
            for gi, (N, C) in per_group.items():
                put(got, prefix, **{"cov_N_%d_%d" % (n, gi): [N], "cov_C_%d_%d" % (n, gi): C})
        Cs, dofs = p.pooled_covariances()
        put(got, prefix, pooled=Cs, dof=dofs)
    del p.calls[:]
    ex, err = p.variance_test(eps=EPS, K=3, N=3)
    put(got, prefix, vt_ex=ex, vt=err, vt_calls=calls_array(p.calls))


# ---- the pilots -------------------------------------------------------------------------------------------------------------------------
def pilot_results(got, prefix, p, calls, printed):
    put(got, prefix, se_c=p.get_covariance_errors(), se_d=p.get_mlmc_variance_errors(), C=p.get_covariances(),
        dV=np.array(p.get_mlmc_variances(), dtype=np.float64), report=report_array(p.pilot_report), calls=calls_array(calls),
        printed=np.frombuffer(printed.encode(), dtype=np.uint8))
    for n in range(p.n_outputs):
        put(got, prefix, **{"se_c_%d" % n: p.get_covariance_error(n), "se_d_%d" % n: p.get_mlmc_variance_error(n)})


def scalar_pilot(got, name, **kw):
    from bluest_amd.blue_models import BLUEProblem
    from bluest_amd.pilot import PilotMixin
    from bluest_amd.pilot_errors import PilotErrorsMixin
    from test_pilot_errors_host import _seeded_class
    calls = []

    class Recorded(_seeded_class(PilotErrorsMixin, PilotMixin, BLUEProblem, heavy=kw.pop("heavy", False))):
        def sampler(self, ls, N=1):
            calls.append((list(ls), int(N)))
            return super().sampler(ls, N)

    printed = io.StringIO()
    with contextlib.redirect_stdout(printed):
        p = Recorded(3, costs=[4.0, 2.0, 1.0], covariance_estimation_samples=20, sample_batch_size=1, verbose=False, **kw)
    pilot_results(got, "pilot_" + name, p, calls, printed.getvalue())


def field_pilot(got, name, **kw):
    from test_field_pilot_errors_host import _classes, _make
    printed = io.StringIO()
    with contextlib.redirect_stdout(printed):
        p = _make(*_classes(), **kw)
    pilot_results(got, "field_pilot_" + name, p, type(p).calls, printed.getvalue())


def unpackers(got):
    from bluest_amd import field_covariances, moments
    sizes, counts = np.array([3, 1, 3, 5, 1], dtype=np.int32), np.array([4, 0, 2, 9, 1], dtype=np.int64)
    tri = sizes * (sizes + 1) // 2
    rng = np.random.RandomState(2)
    first, second = rng.randn(2, sizes.sum()), rng.randn(2, tri.sum())
    for s, (N, f, m) in enumerate(moments._unpacked(counts, sizes, first, second)):
        put(got, "unpacked_moments", **{"N_%d" % s: [N], "first_%d" % s: f, "second_%d" % s: m})
    rows = rng.randn(int(sizes.sum()), 4)
    for with_first in (False, True):
        parts = field_covariances._unpacked(counts, sizes, second[0], second[1], rows if with_first else None)
        for s, part in enumerate(parts):
            put(got, "unpacked_fields_%d" % with_first, **{"N_%d" % s: [part[0]], "second_%d" % s: part[1], "cross_%d" % s: part[2]})
            if with_first:
                put(got, "unpacked_fields_1", **{"first_%d" % s: part[3]})


def record():
    """{key: array}: everything listed in the module's docstring"""
    import gsums_ref
    got = {}
    with restatements():
        for flush in ("default", "each"):
            with flush_sizes(flush):
                for name in gsums_ref.case_names():
                    scalar(got, name, flush)
                for name in ("plain", "stream0", "stream13440", "cov"):
                    field(got, name, flush)
        scalar_pilot(got, "no_tol")
        scalar_pilot(got, "tol", covariance_estimation_tol=0.1)
        scalar_pilot(got, "heavy", covariance_estimation_tol=0.1, heavy=True)
        scalar_pilot(got, "capped", covariance_estimation_tol=0.1, covariance_estimation_max_samples=30)
        field_pilot(got, "no_tol")
        field_pilot(got, "tol", covariance_estimation_tol=0.15)
        field_pilot(got, "capped_samples", covariance_estimation_tol=0.01, covariance_estimation_max_samples=30)
        field_pilot(got, "capped_bytes", covariance_estimation_tol=0.01, covariance_estimation_max_bytes=25 * 3 * 5 * 8 + 7)
    unpackers(got)
    return got


if __name__ == "__main__":
    got = record()
    np.savez_compressed(OUT, **got)
    print("wrote", OUT, "--", len(got), "arrays,", os.path.getsize(OUT), "bytes")
