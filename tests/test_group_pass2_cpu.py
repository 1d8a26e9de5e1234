"""A model of flat_drain's group-only loop (tracer.hip, kGroupsOnly) with single group passes and
with double ones (flat_group_pass2). No GPU.

The loop, as the kernel runs it: a candidate pass whenever nc >= nact; else a group pass whenever
ng >= nact; else, in a drain (th = 1; th = nact means full passes only), a group pass while group
entries are left and then a candidate pass. A single group pass takes the top min(ng, nact) entries;
with double passes a group pass takes the top min(ng, 2 nact) when ng >= nact + th, which is where
the rule would choose a group pass again right after a single one, and counts as two. Each entry
yields 0 to 4 candidates, (entry << 2) | member. Nothing pushes group entries during a drain.

Checked: both forms test the same multiset of entries and make the same multiset of candidates,
count the same group_tests, and with double passes the candidate stack never holds more than 575
entries (kNodeCap = 576: the group-footprint scan keeps its candidates in the node stack). The
single passes' old stack of 320 entries is too small for the double pass: with the cap lowered to
320 the all-hits case overflows, which shows that the model sees an overflow.
"""
import collections
import random

import pytest

NODE_CAP = 576  # tracer.hip kNodeCap
CAND_CAP = 320  # tracer.hip kCandCap


class Overflow(Exception):
    pass


def drain(stack, nact, th, members, double, cand=None, cap=NODE_CAP):
    """One flat_drain call on the group stack `stack` (a list of entries, consumed from its top) and
    the candidate stack `cand` (left over from the call before). members(entry) -> the members the
    exact test lets through. -> dict(tested, cands, group_tests, max_cand, trips, left)."""
    cand = [] if cand is None else cand
    tested, made = [], []
    group_tests = trips = 0
    max_cand = len(cand)
    while True:
        nc, ng = len(cand), len(stack)
        if nc >= nact:
            kind = 0
        elif ng >= nact:
            kind = 1
        elif th == 1:
            kind = 1 if ng else 0 if nc else -1
        else:
            kind = -1
        if kind < 0:
            break
        trips += 1
        if kind == 0:
            del cand[nc - min(nc, nact):]
            continue
        assert nc < nact  # a pass pushes onto fewer than nact entries
        two = double and ng >= nact + th
        m = min(ng, 2 * nact if two else nact)
        top = ng - m
        group_tests += 2 if two else 1
        # lane `rank` takes entry top + rank, then (double) entry top + nact + rank
        lanes = [[stack[top + rank]] + ([stack[top + nact + rank]] if nact + rank < m else [])
                 for rank in range(min(m, nact))]
        del stack[top:]
        for mine in lanes:
            for e in mine:
                tested.append(e)
                new = [(e << 2) | s for s in members(e)]
                made += new
                cand += new
        if len(cand) > cap:
            raise Overflow(f"{len(cand)} candidates, cap {cap}")
        max_cand = max(max_cand, len(cand))
    return dict(tested=tested, cands=made, group_tests=group_tests, max_cand=max_cand,
                trips=trips, left=(list(stack), list(cand)))


def both(entries, nact, th, members):
    one = drain(list(entries), nact, th, members, False, cap=10 ** 9)
    two = drain(list(entries), nact, th, members, True)
    assert collections.Counter(one["tested"]) == collections.Counter(two["tested"])
    assert collections.Counter(one["cands"]) == collections.Counter(two["cands"])
    assert one["group_tests"] == two["group_tests"]
    assert collections.Counter(one["left"][0]) == collections.Counter(two["left"][0])
    assert two["max_cand"] <= NODE_CAP - 1
    assert two["trips"] <= one["trips"]
    return one, two


def yields(kind, seed=0):
    """entry -> members, by the entry alone (both forms must see the same yields)."""
    if kind == "random":
        return lambda e: random.Random(e * 7919 + seed).sample(range(4), random.Random(
            e * 104729 + seed).randint(0, 4))
    n = int(kind)
    return lambda e: list(range(n))


def entries_of(n, seed=1):
    """n distinct group entries (owner << 8 | group), shuffled."""
    r = random.Random(seed)
    return r.sample(range(64 << 8), n)


@pytest.mark.parametrize("kind", ["0", "1", "2", "3", "4", "random"])
def test_boundaries_every_nact(kind):
    """ng = nact, nact + 1, 2 nact, 2 nact + 1 (and one less than each, and 3 nact + 1) at every
    nact from 1 to 64, as a drain and as full passes only."""
    for nact in range(1, 65):
        for ng in sorted({max(nact - 1, 0), nact, nact + 1, 2 * nact - 1, 2 * nact, 2 * nact + 1,
                          3 * nact + 1}):
            for th in (1, nact):
                one, two = both(entries_of(ng, nact), nact, th, yields(kind, nact))
                if th == 1:
                    assert not two["left"][0] and not two["left"][1]
                    assert one["group_tests"] == -(-ng // nact)
                else:
                    assert len(two["left"][0]) == ng % nact
                if ng > nact and (th == 1 or ng >= 2 * nact):
                    assert two["trips"] < one["trips"]


def test_random_heights():
    r = random.Random(12)
    for _ in range(400):
        nact = r.randint(1, 64)
        ng = r.randint(0, 576)
        th = r.choice((1, nact))
        both(entries_of(ng, r.random()), nact, th, yields(r.choice(["random", "4", "0", "2"]),
                                                          r.randint(0, 99)))


def test_slices_carry_the_remainder():
    """The sliced push: full passes only between the slices, the remainder joining the next
    slice's entries, then the drain; candidates left over are carried too."""
    for nact in (1, 2, 7, 33, 64):
        for kind in ("4", "random"):
            res = {}
            for double in (False, True):
                stack, cand, tests, tested, made, top_c = [], [], 0, [], [], 0
                pool = iter(entries_of(16 * 8 * nact, nact))
                for s in range(17):
                    th = nact if s < 16 else 1
                    if s < 16:
                        stack += [next(pool)
                                  for _ in range(random.Random(64 * s + nact).randint(0, 8 * nact))]
                    out = drain(stack, nact, th, yields(kind), double, cand)
                    stack, cand = out["left"]
                    tests += out["group_tests"]
                    tested += out["tested"]
                    made += out["cands"]
                    top_c = max(top_c, out["max_cand"])
                res[double] = (collections.Counter(tested), collections.Counter(made), tests)
                assert not stack and not cand and top_c <= NODE_CAP - 1
            assert res[False] == res[True]


def test_all_hits_reach_the_bound_and_320_is_too_small():
    """64 live lanes, 63 candidates left over, every member of 128 entries accepted: 575 on the
    stack. The same case overflows the single passes' cap of 320."""
    entries = entries_of(128 + 63)
    # 63 candidates left over (fewer than nact: the group pass runs), 191 >= 64 + 1: a double pass
    cand = [(e << 2) for e in range(63)]
    out = drain(list(entries), 64, 1, yields("4"), True, list(cand))
    assert out["max_cand"] == 63 + 2 * 4 * 64 == NODE_CAP - 1
    with pytest.raises(Overflow):
        drain(list(entries), 64, 1, yields("4"), True, list(cand), cap=CAND_CAP)
    # single passes stay within the old cap on the same input
    assert drain(list(entries), 64, 1, yields("4"), False, list(cand), cap=CAND_CAP)["max_cand"] \
        == 63 + 4 * 64 <= CAND_CAP
