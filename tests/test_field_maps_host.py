"""CPU tests of bluest_amd.field_maps: FieldOperator's three ways in, the refusals of MappedFieldsMixin, the hook of
draw_field_values (absent: the shapes and messages of before; present: the per-model widths), the restatement of Part 18
(tests/field_map_ref.py) against a long-double product, the host layout of an operator (bluest_amd/csrc/field_op_layout.hpp,
compiled into a small program of its own) against that restatement, and the declarations of Part 18."""
import os
import re
import subprocess

import numpy as np
import pytest

import field_map_ref as ref
from bluest_amd import field_maps
from bluest_amd.field_maps import FieldOperator, MappedFieldsMixin, map_fields

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("bluest_field_op_create", "bluest_field_op_shape", "bluest_field_op_destroy", "bluest_field_map")


def _bases():
    from bluest_amd.blue_models import BLUEProblem
    from bluest_amd.estimator import SamplingMixin
    from bluest_amd.fields import FieldOutputsMixin
    from bluest_amd.pilot import PilotMixin
    return FieldOutputsMixin, SamplingMixin, PilotMixin, BLUEProblem


def _toy(*bases, weights, operators, M=2, extra=None, **kw):
    """a problem with given covariances: nothing is drawn when it is made"""
    body = {"output_weights": lambda self: weights, "output_operators": lambda self: operators,
            "sampler": lambda self, ls, N=1: [np.zeros(N)] * len(ls)}
    body.update(extra or {})
    Toy = type("Toy", bases, body)
    C = np.eye(M) + 0.5
    return Toy(M, C=[C] * len(weights), costs=np.arange(M, 0, -1.0), n_outputs=len(weights), verbose=False, **kw)


# ---- FieldOperator ---------------------------------------------------------------------------------------------------------------
def test_the_three_ways_in_give_the_same_csr():
    A = np.array([[0.0, 2.0, 0.0, -1.5], [0.0, 0.0, 0.0, 0.0], [4.0, 0.0, 0.25, 0.0]])
    indptr, indices, data = [0, 2, 2, 4], [1, 3, 0, 2], [2.0, -1.5, 4.0, 0.25]

    class Sparse(object):                                               # what scipy.sparse offers, as far as FieldOperator looks
        shape = (3, 4)

        def tocsr(self):
            m = Sparse()
            m.indptr, m.indices, m.data = np.array(indptr, dtype=np.int32), np.array(indices, dtype=np.int64), np.array(data)
            return m

    ops = [FieldOperator((indptr, indices, data), shape=(3, 4)), FieldOperator(A), FieldOperator(Sparse())]
    for op in ops + [FieldOperator(ops[0])]:
        got = op.csr()
        assert op.shape == (3, 4) and op.nnz == 4
        assert [a.dtype for a in got] == [np.int64, np.int32, np.float64]
        assert got[0].tolist() == indptr and got[1].tolist() == indices and got[2].tolist() == data
        assert np.array_equal(np.asarray(ref.dense(op), dtype=np.float64), A)
    # the stored order is kept: neither sorted nor merged
    twice = FieldOperator(([0, 3], [2, 0, 2], [1.0, 2.0, 3.0]), shape=(1, 3))
    assert twice.csr()[1].tolist() == [2, 0, 2] and twice.csr()[2].tolist() == [1.0, 2.0, 3.0]
    with pytest.raises(ValueError):
        twice.csr()[2][0] = 5.0                                         # as stored: read-only


@pytest.mark.parametrize("bad", [
    dict(matrix=([0, 1], [0], [1.0]), shape=(0, 1)), dict(matrix=([0, 1], [0], [1.0]), shape=(1, 0)),
    dict(matrix=([1, 1], [0], [1.0]), shape=(1, 2)), dict(matrix=([0, 2, 1], [0, 1], [1.0, 1.0]), shape=(2, 2)),
    dict(matrix=([0, 1], [2], [1.0]), shape=(1, 2)), dict(matrix=([0, 1], [-1], [1.0]), shape=(1, 2)),
    dict(matrix=([0, 1], [0], [np.inf]), shape=(1, 2)), dict(matrix=([0, 1], [0], [np.nan]), shape=(1, 2)),
    dict(matrix=([0, 2], [0], [1.0]), shape=(1, 2)), dict(matrix=([0, 1, 1], [0], [1.0]), shape=(1, 2)),
    dict(matrix=np.ones(3)), dict(matrix=np.array([[1.0, np.nan]])), dict(matrix=([0, 1], [0], [1.0]), shape=(1, 2**31)),
])
def test_a_matrix_that_is_no_operator_is_refused(bad):
    with pytest.raises(ValueError):
        FieldOperator(**bad)


# ---- the mix-in's refusals -----------------------------------------------------------------------------------------------------------
def test_every_refusal_of_the_mixin():
    from bluest_amd.sap import BLUESTError
    F, S, PM, B = _bases()
    w5, P = np.ones(5), ref.interpolation_1d(3, 5)
    good = _toy(MappedFieldsMixin, F, S, B, weights=[None, w5], operators=[None, [None, (P[:3], P[3])]])
    ops = good._mapped_operators()
    assert ops[0] is None and ops[1][0] is None and isinstance(ops[1][1], FieldOperator) and ops[1][1].shape == (5, 3)
    assert good._mapped_operators() is ops                              # checked once, kept: an operator is uploaded once
    widths, mapper = good._field_batch_hook([1, 0])[1]
    assert widths == [3, 5] and good._field_batch_hook([0])[0] is None
    plain = _toy(MappedFieldsMixin, F, S, B, weights=[None, w5], operators=[None, None])        # nothing declared: as without
    assert plain._field_batch_hook([0, 1]) == [None, None]
    op = FieldOperator(P[:3], shape=P[3])
    refused = {
        "inner products in Python": dict(weights=[None, w5], operators=[None, [None, op]],
                                         extra={"get_models_inner_products": lambda self: [lambda a, b: a * b] * 2}),
        "not M entries": dict(weights=[None, w5], operators=[None, [None, op, op]]),
        "not one entry per output": dict(weights=[None, w5], operators=[None]),
        "different q": dict(weights=[None, w5], operators=[None, [FieldOperator(np.ones((4, 3))), op]]),
        "weights not in the common space": dict(weights=[None, np.ones(3)], operators=[None, [None, op]]),
        "an operator on a number": dict(weights=[None, w5], operators=[[None, op], None]),
        "no operator at all": dict(weights=[None, w5], operators=[None, [None, np.ones(3)]]),
    }
    for why, kw in refused.items():
        with pytest.raises(BLUESTError):
            _toy(MappedFieldsMixin, F, S, B, **kw)
            pytest.fail("not refused: " + why)
    with pytest.raises(BLUESTError, match="FieldOutputsMixin"):
        _toy(MappedFieldsMixin, S, B, weights=[None, w5], operators=[None, [None, op]])
    for name in ("reorder_graph_nodes", "reorder_all_graph_nodes"):
        with pytest.raises(BLUESTError):
            getattr(good, name)()
    with pytest.raises(BLUESTError):                                    # sample files stay refused
        _toy(MappedFieldsMixin, F, PM, B, weights=[None, w5], operators=[None, [None, op]], samplefile="samples.npz")


def test_an_identity_entry_stands_for_d_equal_to_q():
    """model 0 has no operator, so it must deliver q = 5 components: 3 are refused by the width check, with its own d"""
    from bluest_amd.fields import draw_field_values
    from bluest_amd.sap import BLUESTError
    F, S, PM, B = _bases()
    P = ref.interpolation_1d(3, 5)
    p = _toy(MappedFieldsMixin, F, B, weights=[None, np.ones(5)], operators=[None, [None, (P[:3], P[3])]], sample_batch_size=4)
    p.evaluate = lambda ls, samples, N=1: [[np.zeros(4) for _ in ls], [np.zeros((4, 3)) for _ in ls]]
    with pytest.raises(BLUESTError, match=r"model 0 has shape \(4, 3\).*output_operators\(\) declares 5"):
        draw_field_values(p, [0, 1], 4, [1, 5])


# ---- draw_field_values ---------------------------------------------------------------------------------------------------------------
def test_without_the_hook_drawing_is_what_it_was():
    from bluest_amd.fields import draw_field_values
    from bluest_amd.sap import BLUESTError
    F, S, PM, B = _bases()
    p = _toy(F, B, weights=[None, np.ones(3)], operators=None, sample_batch_size=4)
    assert not hasattr(p, "_field_batch_hook")
    seen = []

    def sampler(ls, N=1):
        seen.append((list(ls), N))
        return [np.full(N, float(len(seen)))] * len(ls)
    p.sampler = sampler
    p.evaluate = lambda ls, samples, N=1: [[samples[0] + l for l in ls], [samples[0][:, None] * np.array([1.0, 10.0, 100.0]) + l for l in ls]]
    scalar, field = draw_field_values(p, [0, 1], 6, [1, 3])
    assert seen == [([0, 1], 4), ([0, 1], 2)]
    assert scalar.shape == (6, 2, 1) and field.shape == (6, 2, 3) and np.array_equal(field[5, 1], [3.0, 21.0, 201.0])
    p.evaluate = lambda ls, samples, N=1: [[np.zeros(4) for _ in ls], [np.zeros((4, 2)) for _ in ls]]
    with pytest.raises(BLUESTError, match=r"output_weights\(\) declares 3 component"):
        draw_field_values(p, [0, 1], 4, [1, 3])


def test_with_operators_the_width_check_uses_each_models_own_d(monkeypatch):
    from bluest_amd.fields import draw_field_values
    from bluest_amd.sap import BLUESTError
    F, S, PM, B = _bases()
    P1, P2 = ref.interpolation_1d(3, 5), ref.interpolation_1d(2, 5)
    p = _toy(MappedFieldsMixin, F, B, M=3, weights=[None, np.ones(5)], operators=[None, [None, (P1[:3], P1[3]), (P2[:3], P2[3])]],
             sample_batch_size=4)
    widths = {0: 5, 1: 3, 2: 2}
    calls = []

    def sampler(ls, N=1):
        calls.append((list(ls), N))
        return [np.arange(N) + 10.0 * len(calls)] * len(ls)
    p.sampler = sampler
    wrong = {"model": None}
    poison = [True]

    def evaluate(ls, samples, N=1):
        field = [samples[0][:, None] + np.arange(widths[l] + (1 if l == wrong["model"] else 0)) for l in ls]
        if poison and len(calls) == 2:
            poison.pop()
            field[1][0, 0] = np.inf                                     # a non-finite RAW value: the batch is drawn again, unmapped
        return [[samples[0] + l for l in ls], field]
    p.evaluate = evaluate
    mapped = []

    def stand_in(values, operators, **kw):                              # the GPU call replaced by its restatement
        mapped.append([v.shape for v in values])
        return ref.map_fields(values, operators)
    monkeypatch.setattr(field_maps, "map_fields", stand_in)
    scalar, field = draw_field_values(p, [2, 0, 1], 6, [1, 5])
    assert calls == [([2, 0, 1], 4), ([2, 0, 1], 2), ([2, 0, 1], 2)]
    assert mapped == [[(4, 2), (4, 5), (4, 3)], [(2, 2), (2, 5), (2, 3)]]           # every finite batch once, as it arrived
    assert scalar.shape == (6, 3, 1) and field.shape == (6, 3, 5)
    assert np.array_equal(field[0, 1], 10.0 + np.arange(5)) and np.array_equal(field[0, 0], 10.0 + np.linspace(0, 1, 5))
    assert np.array_equal(field[4, 2], 30.0 + np.linspace(0, 2, 5))
    for model, d in ((1, 3), (2, 2), (0, 5)):
        wrong["model"] = model
        with pytest.raises(BLUESTError, match=r"of model %d has shape \(4, %d\).*output_operators\(\) declares %d component" % (model, d + 1, d)):
            draw_field_values(p, [2, 0, 1], 4, [1, 5])


# ---- the restatement -----------------------------------------------------------------------------------------------------------------
def test_the_restatement_agrees_with_a_long_double_product():
    rng = np.random.RandomState(7)
    P = ref.interpolation_1d(9, 17)
    print("interpolation:", ref.self_check(P, rng.randn(3, 9)))
    op = ref.random_operator(rng, 6, 40, [0, 1, 2, 40, 700])
    op = (op[0], op[1], rng.randn(len(op[2])), op[3])                   # general coefficients: the exact fma
    print("general rows up to 700 entries:", ref.self_check(op, rng.randn(2, 40)))
    long = ref.random_operator(rng, 3, 50, [511, 513, 1100])
    y = ref.data26(rng, 2, 50)
    print("exact products, rows of 511 / 513 / 1100:", ref.self_check(long, y, exact_products=True))
    assert ref.same_bits(ref.apply(long, y, exact_products=True), ref.apply(long, y))          # the two fmas are one where products are exact
    assert ref.same_bits(ref.map_fields([y, y[:, :3]], [long, None], exact_products=True)[:, 1], y[:, :3])


# ---- the host layout (plain C++, compiled on its own) --------------------------------------------------------------------------------
def _hex(values):
    return " ".join(float(v).hex() for v in np.asarray(values, dtype=np.float64).reshape(-1))


def test_the_host_layout_applies_an_operator_as_the_restatement_does(tmp_path):
    exe = str(tmp_path / "field_op_layout")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tests", "field_op_layout_main.cpp"), "-o", exe])
    rng = np.random.RandomState(11)
    strip = 8                                                            # a short strip: long rows at a size the exact fma walks
    cases = [(ref.random_operator(rng, q, d, lengths), N) for q, d, lengths, N in (
        (1, 1, [1], 1), (63, 7, [0, 1, 2, 7, 8], 2), (64, 7, [8, 9, 0, 20], 2), (130, 11, [3, 0, 9, 8, 1, 17, 2], 3))]
    cases = [((op[0], op[1], rng.randn(len(op[2])), op[3]), rng.randn(N, op[3][1])) for op, N in cases]
    # eleven rows over all of 20 columns with a short row among them: long rows with one column sequence, bundled 2 + 1 + 8
    dense = (np.array([0, 20, 40, 60, 80, 100, 120, 140, 160, 180, 200, 203, 223]), np.concatenate([np.tile(np.arange(20), 10), [4, 4, 1], np.arange(20)]),
             rng.randn(223), (12, 20))
    dense[1][45] = 7                                                    # row 2 names another column at its sixth place: it stands alone
    cases.append((dense, rng.randn(2, 20)))
    bad = [((np.array([0, 1]), np.array([3]), np.array([1.0]), (1, 3)), "outside"), ((np.array([1, 1]), np.array([0]), np.array([1.0]), (1, 3)), "must be 0"),
           ((np.array([0, 2, 1]), np.array([0, 1]), np.ones(2), (2, 3)), "decreases"), ((np.array([0, 1]), np.array([0]), np.array([np.inf]), (1, 3)), "finite"),
           ((np.array([0]), np.array([], dtype=int), np.array([]), (0, 3)), "at least one row")]
    text = []
    for (indptr, idx, data, (q, d)), y in cases + [(op, np.zeros((0, 3))) for op, _ in bad]:
        text.append("%d %d %d %d %d\n%s\n%s\n%s\n%s\n" % (q, d, len(idx), len(y), strip, " ".join(map(str, indptr)), " ".join(map(str, idx)), _hex(data),
                                                         _hex(y)))
    path = tmp_path / "cases.txt"
    path.write_text("".join(text))
    lines = subprocess.check_output([exe, str(path)]).decode().splitlines()
    old, ref.STRIP = ref.STRIP, strip
    try:
        for op, y in cases:
            head = lines.pop(0).split()
            lens = np.diff(op[0])
            assert head[0] == "OK" and int(head[1]) == (op[3][0] + 63) // 64 and int(head[2]) == int((lens > strip).sum())
            slots = sum(64 * max([n for n in lens[t:t + 64] if n <= strip], default=0) for t in range(0, op[3][0], 64))
            assert int(head[3]) == slots
            rows = [tuple(op[1][op[0][r]:op[0][r + 1]]) for r in range(op[3][0]) if lens[r] > strip]
            bundles, held = 0, 0
            for j, row in enumerate(rows):                              # at most 8 consecutive long rows with the first one's columns
                if j == 0 or held == 8 or row != first:
                    bundles, held, first = bundles + 1, 0, row
                held += 1
            assert int(head[4]) == bundles and (op is not dense or bundles == 3)
            got = np.array([[float.fromhex(v) for v in lines.pop(0).split()] for _ in range(len(y))])
            assert ref.same_bits(got, ref.apply(op, y))
    finally:
        ref.STRIP = old
    for (_, word), line in zip(bad, lines):
        assert line.startswith("ERR") and word in line, line
    assert len(lines) == len(bad)


# ---- the ABI -------------------------------------------------------------------------------------------------------------------------
def test_part_18_declares_the_four_symbols_and_the_binding_lists_them():
    from bluest_amd import _lib
    text = open(os.path.join(ROOT, "include", "bluest_hip.h")).read()
    part = text[text.index("Part 18 --"):]
    code = re.sub(r"/\*.*?\*/", "", part[part.index("*/"):], flags=re.S)
    assert sorted(set(re.findall(r"\b(bluest_[a-z0-9_]+)\s*\(", code))) == sorted(SYMBOLS)
    assert re.search(r"#define\s+BLUEST_FIELD_MAP_STRIP\s+%d\b" % field_maps.BLUEST_FIELD_MAP_STRIP, code) and ref.STRIP == field_maps.BLUEST_FIELD_MAP_STRIP
    assert "typedef struct bluest_field_op *bluest_field_op_t;" in code
    assert [len(_lib.SIGNATURES[s]) for s in SYMBOLS] == [6, 4, 1, 7]
    L = _lib.lib()
    assert all(hasattr(L, s) for s in SYMBOLS) and L.bluest_abi_version() == 1


def test_the_argument_checks_of_map_fields_need_no_device():
    import torch
    from bluest_amd import _lib
    op = FieldOperator(np.ones((2, 3)))
    for values, operators in (([np.ones((4, 3))], [op, op]), ([], []), ([np.ones((4, 2))], [op]), ([np.ones((4, 3)), np.ones((5, 2))], [op, None]),
                              ([np.ones((4, 3)), np.ones((4, 3))], [op, None]), ([np.ones(3)], [op]), ([np.ones((4, 3))], [np.ones((2, 3))]),
                              ([np.ones((4, 3)), np.ones((4, 3))], [op, FieldOperator(np.ones((4, 3)))])):
        with pytest.raises(ValueError):
            map_fields(values, operators)
    if not torch.cuda.is_available():                                   # and there is no CPU path
        with pytest.raises(_lib.BluestHipError):
            map_fields([np.ones((4, 3))], [op])
