"""The LDS schedule of the 8-wave posterior kernel (csrc/post_wide_sched.h),
walked on the host through bo_post_wide_schedule: the same inline functions
the kernel indexes its U ring with.

For every segment length 1 .. 40 and both walk directions:
  * both halves of the workgroup execute the same number of barriers;
  * no LDS stage is written in a barrier interval in which either half reads
    it, and every read finds the step it wants: the last store to that stage,
    by BOTH halves (each stores half of the rows), lies in an earlier interval
    and holds that step;
  * every (step, k-slice) is read exactly once and multiplied exactly once per
    half, read before it is multiplied, in the walk's order, at the walk's rows.
"""
import ctypes

import pytest

from botorch_amd import _lib

READ, STORE, MFMA = 0, 1, 2
NSTEPS = range(1, 41)


def _schedule(nsteps, half, rev):
    """(barriers, [(interval, kind, step, slice, stage, k0), ...] in program order)."""
    cap = 20 * (nsteps + 2)
    ev = (ctypes.c_int * (6 * cap))()
    nb, ne = ctypes.c_int(), ctypes.c_int()
    rc = _lib.lib().bo_post_wide_schedule(nsteps, half, rev, cap, ctypes.byref(nb), ctypes.byref(ne),
                                          ctypes.cast(ev, ctypes.c_void_p))
    assert rc == 0
    assert 0 < ne.value <= cap
    return nb.value, [tuple(ev[6 * i:6 * i + 6]) for i in range(ne.value)]


@pytest.mark.parametrize("rev", [0, 1], ids=["ascending", "descending"])
def test_both_halves_count_the_same_barriers(rev):
    for nsteps in NSTEPS:
        (b0, e0), (b1, e1) = _schedule(nsteps, 0, rev), _schedule(nsteps, 1, rev)
        assert b0 == b1
        # interval -1 (prologue) .. b - 2, a barrier after each of them (the
        # last interval may be empty: it holds only the late half's trailing units)
        for ev in (e0, e1):
            js = [e[0] for e in ev]
            assert js == sorted(js), "events are in program order"
            assert min(js) == -1 and b0 - 3 <= max(js) <= b0 - 2


@pytest.mark.parametrize("rev", [0, 1], ids=["ascending", "descending"])
def test_no_stage_is_written_while_it_may_be_read(rev):
    for nsteps in NSTEPS:
        halves = [_schedule(nsteps, h, rev)[1] for h in (0, 1)]
        stores = [[e for e in ev if e[1] == STORE] for ev in halves]
        # both halves store their share of every step, in the same interval
        assert [(e[0], e[2], e[4]) for e in stores[0]] == [(e[0], e[2], e[4]) for e in stores[1]]
        for ev in halves:
            for (j, kind, step, sl, stage, _) in ev:
                if kind != READ:
                    continue
                for st in stores:
                    assert all(not (w[4] == stage and w[0] == j) for w in st), \
                        f"nsteps {nsteps}: stage {stage} written in interval {j} while read"
                    before = [w for w in st if w[4] == stage and w[0] < j]
                    assert before, f"nsteps {nsteps}: stage {stage} read before it was written"
                    # a stage holds the steps of one super-step: what the last
                    # storing interval before the read put there
                    held = {w[2] for w in before if w[0] == before[-1][0]}
                    assert step in held, \
                        f"nsteps {nsteps}: step {step} slice {sl} read from a stage holding {held}"


@pytest.mark.parametrize("rev", [0, 1], ids=["ascending", "descending"])
def test_every_slice_is_read_once_and_multiplied_once(rev):
    for nsteps in NSTEPS:
        want = [(s, k) for s in range(nsteps) for k in range(4)]
        for half in (0, 1):
            _, ev = _schedule(nsteps, half, rev)
            reads = [(e[2], e[3]) for e in ev if e[1] == READ]
            mfmas = [(e[2], e[3]) for e in ev if e[1] == MFMA]
            assert sorted(reads) == want, f"nsteps {nsteps} half {half}: reads"
            assert mfmas == want, f"nsteps {nsteps} half {half}: MFMA order"
            pos = {(e[1], e[2], e[3]): i for i, e in enumerate(ev)}
            for s, k in want:
                assert pos[(READ, s, k)] < pos[(MFMA, s, k)]
            stage_of = {}
            for e in ev:
                s = min(e[2], nsteps - 1)  # a ragged last stage repeats the last step's rows
                assert e[5] == 16 * ((nsteps - 1 - s) if rev else s)
                assert stage_of.setdefault(e[2], e[4]) == e[4], "a step lives in one stage"


def test_the_late_half_never_leads_and_trails_by_a_constant():
    """After every interval but the last the late half is the same number of
    k-slices behind the early half (at most one stage of two steps: it reads
    at most one stage back), and both finish the segment."""
    for nsteps in NSTEPS:
        (nb, e0), (_, e1) = _schedule(nsteps, 0, 0), _schedule(nsteps, 1, 0)
        done0 = done1 = 0
        gaps = set()
        for j in range(0, nb - 1):
            done0 += sum(1 for e in e0 if e[0] == j and e[1] == MFMA)
            done1 += sum(1 for e in e1 if e[0] == j and e[1] == MFMA)
            assert 0 <= done0 - done1 <= 8
            if done0 < 4 * nsteps:
                gaps.add(done0 - done1)
        assert len(gaps) <= 1
        assert done0 == done1 == 4 * nsteps


def test_bad_arguments_are_refused():
    nb, ne = ctypes.c_int(), ctypes.c_int()
    f = _lib.lib().bo_post_wide_schedule
    assert f(0, 0, 0, 0, ctypes.byref(nb), ctypes.byref(ne), None) != 0
    assert f(4, 2, 0, 0, ctypes.byref(nb), ctypes.byref(ne), None) != 0
    assert f(4, 1, 0, 0, ctypes.byref(nb), ctypes.byref(ne), None) == 0 and ne.value > 0
