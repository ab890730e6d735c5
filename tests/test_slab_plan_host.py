"""
The slab planner of the ragged sample-sum calls (bluest_amd/csrc/slab_plan.hpp) without a GPU: tests/slab_plan_main.cpp, which
includes nothing but that header, is compiled with g++ and run once over all cases; its plans must equal, number for number, the
packing rule restated here, and keep the properties the entry points rely on (a slab boundary never shows in a result because
every piece but a segment's last is a whole number of chunks).
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNK = 128
DEFAULT_BUDGET = 256 << 20
MID_BUDGET = 3 * 128 * 7 * 8 * 2 + 1000          # the odd budget of the GPU tests: a segment ends in the middle of a slab
COUNTS = [0, 1, 127, 128, 129, 64 * 128 + 5]


def align256(x):
    return (x + 255) // 256 * 256


def expected_plan(segs, budget):
    """segs: [(count, row_bytes, staged)].  The rule: the budget in effect is at least the widest chunk of the call + 256; the
    staged segments are laid one after the other, every piece at the next multiple of 256 bytes of its slab (or at the budget,
    if that comes first); a piece is the rest of its segment if that fits the slab, else as many whole chunks as fit; if not
    one fits, the slab is closed and the next one starts empty."""
    budget = max(budget, CHUNK * max(rb for _, rb, _ in segs) + 256)
    pieces, used_per_slab, used, slab = [], [], 0, 0
    for seg, (count, rb, staged) in enumerate(segs):
        first = 0
        while staged and first < count:
            room = (budget - used) // rb
            if room < count - first:
                room = room // CHUNK * CHUNK
            if room == 0:
                used_per_slab.append(used)
                used, slab = 0, slab + 1
                continue
            rows = min(room, count - first)
            pieces.append((seg, first, rows, used, slab))
            used = min(budget, align256(used + rows * rb))
            first += rows
    if pieces:
        used_per_slab.append(used)
    return budget, max(used_per_slab, default=0), used_per_slab, pieces


def cases():
    rows = {"L3": 3 * 8, "L7x2": 7 * 8 * 2, "L32x2": 32 * 8 * 2, "L32d63": 32 * 63 * 8, "L1": 8}
    lists = {
        # every count at one narrow row whose pieces end off the 256-byte grid (a whole chunk is a multiple of 1024 bytes)
        "counts_L3": [(n, rows["L3"], 1) for n in COUNTS],
        "counts_L7x2": [(n, rows["L7x2"], 1) for n in COUNTS],
        "widest_n_out2": [(n, rows["L32x2"], 1) for n in (129, 64 * 128 + 5, 1)],
        "widest_d63": [(n, rows["L32d63"], 1) for n in (127, 128, 129, 64 * 128 + 5)],
        "ragged": [(n, rb, 1) for n, rb in zip(COUNTS + COUNTS[::-1], [8, 24, 112, 512, 16128, 40, 56, 8, 2016, 24, 112, 8])],
        # device-resident segments get no piece; a device segment wider than every staged one still raises the budget in effect
        "mixed": [(300, rows["L7x2"], 1), (5000, rows["L32d63"], 0), (129, rows["L3"], 1), (0, rows["L1"], 0), (8197, rows["L7x2"], 0),
                  (8197, rows["L7x2"], 1), (1, rows["L1"], 1)],
        "none_staged": [(500, rows["L7x2"], 0), (0, rows["L3"], 0), (129, rows["L32x2"], 0)],
        "one_empty": [(0, rows["L3"], 0)],
    }
    return [("%s-%d" % (name, budget), segs, budget) for name, segs in lists.items() for budget in (1, MID_BUDGET, DEFAULT_BUDGET)]


CASES = cases()


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    """name -> (budget in effect, stage_bytes, [bytes per slab], [(seg, first, rows, at, slab)]) as the C++ planner gives them"""
    exe = str(tmp_path_factory.mktemp("slab_plan") / "slab_plan_main")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "bluest_amd", "csrc"),
                    os.path.join(ROOT, "tests", "slab_plan_main.cpp"), "-o", exe], check=True, capture_output=True, text=True, timeout=120)
    text = "".join("%d %d %d\n%s" % (len(segs), CHUNK, budget, "".join("%d %d %d\n" % s for s in segs)) for _, segs, budget in CASES)
    out = subprocess.run([exe], input=text, check=True, capture_output=True, text=True, timeout=60).stdout.splitlines()
    got, at = {}, 0
    for name, _, _ in CASES:
        head = out[at].split()
        assert head[0] == "plan"
        budget, stage_bytes, n_slabs, n_pieces = (int(x) for x in head[1:])
        used = [int(x) for x in out[at + 1].split()[1:]]
        assert len(used) == n_slabs
        pieces = [tuple(int(x) for x in line.split()[1:]) for line in out[at + 2:at + 2 + n_pieces]]
        assert all(line.startswith("piece ") for line in out[at + 2:at + 2 + n_pieces])
        got[name] = (budget, stage_bytes, used, pieces)
        at += 2 + n_pieces
    assert at == len(out)
    return got


@pytest.mark.parametrize("name,segs,budget", CASES, ids=[c[0] for c in CASES])
def test_plan_equals_the_rule(plans, name, segs, budget):
    assert plans[name] == expected_plan(segs, budget)


@pytest.mark.parametrize("name,segs,budget", CASES, ids=[c[0] for c in CASES])
def test_plan_properties(plans, name, segs, budget):
    effective, stage_bytes, used, pieces = plans[name]
    assert effective >= budget and all(effective >= CHUNK * rb + 256 for _, rb, _ in segs)
    for seg, (count, rb, staged) in enumerate(segs):
        mine = [p for p in pieces if p[0] == seg]
        if not staged or count == 0:
            assert mine == []                                   # device-resident or empty: no piece
            continue
        assert mine[0][1] == 0 and mine[-1][1] + mine[-1][2] == count
        for a, b in zip(mine, mine[1:]):
            assert a[1] + a[2] == b[1]                          # the pieces tile [0, count) in order
        assert all(p[2] > 0 for p in mine) and all(p[2] % CHUNK == 0 for p in mine[:-1])
    assert [p for p in pieces] == sorted(pieces, key=lambda p: (p[0], p[1]))        # segment by segment, rows ascending
    end = {}
    for seg, first, rows, at, slab in pieces:
        assert at % 256 == 0
        assert at >= end.get(slab, 0)                           # the pieces of a slab do not overlap
        end[slab] = at + rows * segs[seg][1]
        assert end[slab] <= effective                           # no piece runs past the budget in effect
    slabs = [p[4] for p in pieces]
    assert slabs == sorted(slabs) and sorted(set(slabs)) == list(range(len(used)))  # ascending, no gap, no empty slab
    assert all(end[k] <= used[k] <= effective for k in range(len(used)))
    assert stage_bytes == max(used, default=0)
    if budget == 1 and pieces:                                  # room for one widest chunk and 256 bytes: never for two chunks
        widest = max(rb for _, rb, _ in segs)
        per_slab = [sum(p[2] for p in pieces if p[4] == k and segs[p[0]][1] == widest) for k in range(len(used))]
        assert max(per_slab) <= CHUNK + 256 // widest < 2 * CHUNK


def test_cases_cover_what_they_must(plans):
    """the case list itself: a segment that ends in the middle of a slab, several slabs, several pieces per segment"""
    _, _, used, pieces = plans["counts_L7x2-%d" % MID_BUDGET]
    assert len(used) > 3
    assert any(a[4] == b[4] and a[0] != b[0] for a, b in zip(pieces, pieces[1:]))       # two segments share a slab
    assert any(a[4] != b[4] and a[0] == b[0] for a, b in zip(pieces, pieces[1:]))       # a segment goes on in the next slab
    assert plans["none_staged-1"][1:] == (0, [], []) and plans["one_empty-1"][1:] == (0, [], [])
    assert len(plans["ragged-%d" % DEFAULT_BUDGET][2]) == 1                             # the default budget holds all of it
