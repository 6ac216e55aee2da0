"""Host logic of kernels._LadderRing (the gradient path's deferred ladder
outcome for qEHVI / qNEHVI) with stand-in pinned blocks and events: a
backward settles its own forward only, a block that comes round again
reports the forward that left it pending (one ring behind), the poll reports
the pending ones oldest first, and outcomes raise / warn as the per-member
psd_safe_cholesky checks would."""
import warnings

import pytest

from botorch_amd import kernels
from botorch_amd.exceptions import NotPSDError, NumericalWarning


class _Block:
    def __init__(self):
        self.words = [0.0] * 16

    def arm(self, m):
        for i in range(2 * m):
            self.words[i] = 0.0
        return [(i, i) for i in range(m)]


class _Event:
    def __init__(self):
        self.recorded = 0
        self.synced = 0

    def record(self, stream=None):
        self.recorded += 1

    def synchronize(self):
        self.synced += 1


def _ring():
    r = kernels._LadderRing.__new__(kernels._LadderRing)
    r.dev = None
    r.blocks = [_Block() for _ in range(kernels._LadderRing.N)]
    r.events = [_Event() for _ in range(kernels._LadderRing.N)]
    r.pending = [None] * kernels._LadderRing.N
    r.next = 0
    r.gen = 0
    return r


def test_backward_settles_its_own_forward():
    r = _ring()
    tok, words = r.take(3, "qEHVI posterior root")
    assert len(words) == 3
    r.blocks[tok[0]].words[3] = 1e-6  # member 1 jittered
    with pytest.warns(NumericalWarning, match="1.0e-06"):
        r.settle(tok)
    assert r.pending[tok[0]] is None and r.events[tok[0]].synced == 1
    r.settle(tok)  # settled once: nothing more


def test_stale_token_does_not_settle_a_newer_forward():
    r = _ring()
    tok0, _ = r.take(2, "a")
    for _ in range(kernels._LadderRing.N):  # the ring comes round: tok0's block reused
        tok, _ = r.take(2, "b")
    assert tok[0] == tok0[0] and tok[1] != tok0[1]
    r.blocks[tok[0]].words[0] = 1.0  # the NEWER forward failed
    r.settle(tok0)  # the old token: no read, no raise
    assert r.pending[tok[0]] is not None
    with pytest.raises(NotPSDError, match="b"):
        r.settle(tok)


def test_block_coming_round_reports_the_forward_left_pending():
    r = _ring()
    tok0, _ = r.take(1, "first")
    r.blocks[tok0[0]].words[0] = 1.0  # its backward never ran
    for _ in range(kernels._LadderRing.N - 1):
        r.take(1, "later")
    with pytest.raises(NotPSDError, match="first"):
        r.take(1, "wraps")  # the reuse of tok0's block reads it first
    assert r.pending[tok0[0]] is None


def test_released_block_is_never_waited_on_or_read():
    """A forward that raised between take() and record() gives its block back:
    no event stands behind it, so the wrap-around, settle and settle_all must
    neither wait on that slot's event nor read its words."""
    r = _ring()
    tok, _ = r.take(2, "raised")
    r.release(tok)
    assert r.pending[tok[0]] is None
    r.blocks[tok[0]].words[0] = 1.0  # a stale failure word in the released block
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        r.settle(tok)  # the released token: a no-op
        r.settle_all()
        for _ in range(kernels._LadderRing.N):  # round the ring, onto that block again
            later, _ = r.take(2, "later")
        assert later[0] == tok[0] and r.events[tok[0]].synced == 0
        r.settle(tok)  # still a no-op: the block now belongs to a newer forward
    assert r.pending[tok[0]] is not None and r.events[tok[0]].synced == 0


def test_release_of_a_stale_token_leaves_the_newer_forward_pending():
    r = _ring()
    tok0, _ = r.take(1, "a")
    r.settle(tok0)
    for _ in range(kernels._LadderRing.N):
        tok, _ = r.take(1, "b")
    assert tok[0] == tok0[0]
    r.release(tok0)
    assert r.pending[tok[0]] is not None


class _Ctx:
    ladder = "unset"


def _policy(monkeypatch, capture=False, sync=False):
    ring, block = _ring(), _Block()
    monkeypatch.setattr(kernels, "ladder_ring", lambda dev: ring)
    monkeypatch.setattr(kernels, "pinned_status", lambda dev: block)
    monkeypatch.setattr(kernels, "_CAPTURE", {0: None} if capture else {})
    monkeypatch.setattr(kernels, "SYNC_LADDER", sync)
    monkeypatch.setattr(kernels.torch.cuda, "current_stream", lambda dev=None: None)  # no GPU here
    return ring, block


@pytest.mark.parametrize("need_grad,defer_only,capture,sync,M,route", [
    (True, False, False, False, 3, "ring"), (True, True, False, False, 8, "ring"),
    (False, True, False, False, 3, "defer"), (False, False, False, False, 3, "pinned"),
    (True, False, False, True, 3, "pinned"), (False, True, False, True, 3, "pinned"),
    (True, False, True, False, 3, "device"), (False, True, True, False, 3, "device"),
    (True, True, False, False, 9, "device"), (False, True, False, False, 9, "defer")])
def test_member_ladder_routes(monkeypatch, need_grad, defer_only, capture, sync, M, route):
    """kernels.member_ladder: which of ring / deferred / pinned block / device
    tensors a forward over M members takes, and what finish() then does."""
    ring, block = _policy(monkeypatch, capture, sync)
    seen = []
    monkeypatch.setattr(kernels, "raise_not_psd_members", lambda ps, m, dev, what: seen.append(("pinned", ps, m)))
    monkeypatch.setattr(kernels, "raise_not_psd_many", lambda pairs, what: seen.append(("device", len(pairs))))
    monkeypatch.setattr(kernels, "raise_not_psd_deferred",
                        lambda i, j, what: seen.append(("defer", i.numel(), j.numel())))
    import torch
    lad = kernels.member_ladder("cuda:0", M, need_grad, "x", defer_forward_only=defer_only)
    assert (lad.words is None) == (route in ("defer", "device"))
    ctx = _Ctx()
    info, jit = torch.zeros(M, 2, dtype=torch.int32), torch.zeros(M, 2, dtype=torch.float64)
    with lad:
        lad.finish(ctx, info, jit)
    if route == "ring":
        assert ctx.ladder[0] is ring and ring.pending[ctx.ladder[1][0]] is not None and not seen
        assert ring.events[ctx.ladder[1][0]].recorded == 1
    else:
        assert ctx.ladder is None and all(p is None for p in ring.pending)
        assert seen == [{"pinned": ("pinned", block, M), "device": ("device", M),
                         "defer": ("defer", 2 * M, 2 * M)}[route]]


def test_member_ladder_releases_the_block_of_a_forward_that_raises(monkeypatch):
    ring, _ = _policy(monkeypatch)
    with pytest.raises(ValueError):
        with kernels.member_ladder("cuda:0", 2, True, "x") as lad:
            assert ring.pending[lad.token[0]] is not None
            raise ValueError("host code failed")
    assert all(p is None for p in ring.pending)
    # a forward that finished keeps its block pending for the backward
    ctx = _Ctx()
    with pytest.raises(ValueError):
        with kernels.member_ladder("cuda:0", 2, True, "x") as lad:
            lad.finish(ctx, None, None)
            raise ValueError("after the record")
    assert ring.pending[ctx.ladder[1][0]] is not None


def test_settle_all_oldest_first_and_member_order():
    r = _ring()
    t1, _ = r.take(2, "one")
    t2, _ = r.take(2, "two")
    r.blocks[t1[0]].words[1] = 1e-8
    r.blocks[t2[0]].words[2] = 1.0  # member 1 of the second forward failed
    with warnings.catch_warnings(record=True) as ws:
        warnings.simplefilter("always")
        with pytest.raises(NotPSDError, match="two"):
            r.settle_all()
    assert any(issubclass(w.category, NumericalWarning) for w in ws)  # "one" reported first
    assert all(p is None for p in r.pending)
