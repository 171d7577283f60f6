"""The flat speculation's replica ranges from a sample (merge.hip k_pre_sample).

A fresh tree's flat batch is merged with the replica ranges folded from its
first and last S ops only (CRDTM_PRE_SAMPLE, ops per end); the full pre-pass
behind the sample returns at once on the device when the sampled ranges sum
to n. Sampled ranges are sub-ranges of the exact ones, and a batch the
speculation keeps is dense and duplicate-free, so a sample that sums to n has
found the exact ranges of every batch that is kept: the claim's counters
decide, and a merge they do not confirm keeps nothing and takes the general
path (exact ranges, no second speculation). crdtm_result.flags carries
CRDTM_FLAG_RANGES_SAMPLED when a merge was kept on sampled ranges.

Every case states, in numpy on the host arrays, which tier its batch reaches
(the sample's total against n and against the exact total) before it calls
the engine, and compares with the oracle as test_flat_speculation_shapes does:
code / err_index, the summaries, and for a merge that succeeds the log, the
document, n_applied and the status array.
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from crdtm import _native as N  # noqa: E402
from crdtm.tree import CRDTree  # noqa: E402
from parity_util import (engine_log, engine_summary, oracle_apply_arrays, oracle_log, oracle_summary,  # noqa: E402
                         oracle_visible_vals)

S_DEFAULT = 32768  # (merge.hip PRE_SAMPLE)
REP_SPEC = 256     # (merge.hip: replica ids the speculation's range table holds)
TWO53 = 1 << 53


def _arrays(ops):
    """[(kind, ts, path list, val)] -> packed host arrays."""
    kind = np.array([o[0] for o in ops], np.uint8)
    ts = np.array([o[1] for o in ops], np.int64)
    off = np.zeros(len(ops) + 1, np.uint32)
    off[1:] = np.cumsum([len(o[2]) for o in ops])
    path = np.array([k for o in ops for k in o[2]] or [0], np.int64)[:int(off[-1])]
    val = np.array([o[3] for o in ops], np.uint32)
    return dict(kind=kind, ts=ts, path_off=off, path=path, val=val)


@functools.lru_cache(maxsize=None)
def _stream(n, replicas, window, seed):
    s = N.synth(n_ops=n, replicas=replicas, window=window, seed=seed)
    return tuple((0, int(s["ts"][i]), (int(s["path"][i]),), int(s["val"][i])) for i in range(n))


def _base():
    """The 20,000-op stream of 64 replicas: 512 ops per end find every exact
    range, 64 / 128 / 256 per end do not."""
    return [(k, t, list(p), v) for k, t, p, v in _stream(20000, 64, 256, 7)]


def _range_total(ts):
    """Sum of the per-replica counter range sizes over the timestamps the
    pre-pass folds (0 < ts < 2^53), and whether it saw one it refuses."""
    ts = np.asarray(ts, np.int64)
    refused = bool(np.any((ts < 0) | (ts >= TWO53)))
    t = ts[(ts > 0) & (ts < TWO53)]
    rep, ctr = t >> 32, t & 0xFFFFFFFF
    refused |= bool(np.any(rep >= REP_SPEC))
    total = 0
    for r in np.unique(rep):
        c = ctr[rep == r]
        total += int(c.max()) - int(c.min()) + 1
    return total, refused


def _tiers(ts, S):
    """(sampled, sample total, exact total): what k_pre_sample decides for a
    batch of these timestamps at S ops per end. sampled: the device takes the
    sampled ranges (pre_sampled = 1)."""
    n = len(ts)
    S = (S + 1) & ~1
    exact, _ = _range_total(ts)
    if n <= 2 * S:
        return False, exact, exact
    t = (n - S) & ~1
    total, refused = _range_total(np.concatenate([ts[:S], ts[t:]]))
    return total == n and not refused, total, exact


def _merge_and_compare(ops, et=None, closed=True):
    """One merge on a fresh tree against the oracle; returns the result and
    the oracle's code. closed: a merge that succeeds took the closed form."""
    s = _arrays(ops)
    n = len(ops)
    assert int(s["path_off"][-1]) == n  # (the speculation's trigger)
    ot, rc, oerr = oracle_apply_arrays(s, n)
    et = et or CRDTree.init(0)
    st = np.full(n, 9, np.uint8)
    res = et.apply_arrays(s, n, status=st)
    assert (res.code, res.err_index if rc else -1) == (rc, oerr if rc else -1), (res.code, res.err_index, rc, oerr)
    assert engine_summary(et) == oracle_summary(ot)
    if rc == 0:
        assert not closed or res.path_taken == N.PATH_CLOSED_FORM
        assert engine_log(et, 0) == oracle_log(ot, 0)
        assert np.array_equal(et.document_handles(), oracle_visible_vals(ot))
        assert res.n_applied == int(np.sum(st == 0))
    else:
        assert not res.flags & N.FLAG_RANGES_SAMPLED
    from oracle.oracle import lib as olib
    olib().orc_free(ot)
    return res, rc


def _ts(ops):
    return np.array([o[1] for o in ops], np.int64)


def test_sample_suffices(monkeypatch):
    monkeypatch.setenv("CRDTM_PRE_SAMPLE", "512")
    ops = _base()
    sampled, total, exact = _tiers(_ts(ops), 512)
    assert sampled and total == exact == len(ops)
    res, rc = _merge_and_compare(ops)
    assert rc == 0 and res.flags & N.FLAG_RANGES_SAMPLED


@pytest.mark.parametrize("S", [64, 128, 256])
def test_sample_falls_short_on_the_device(monkeypatch, S):
    """The sample's total is not n: the full pass behind it lays out the exact
    ranges and the merge is kept on those."""
    monkeypatch.setenv("CRDTM_PRE_SAMPLE", str(S))
    ops = _base()
    sampled, total, exact = _tiers(_ts(ops), S)
    assert not sampled and total != len(ops) and exact == len(ops)
    res, rc = _merge_and_compare(ops)
    assert rc == 0 and not res.flags & N.FLAG_RANGES_SAMPLED


@pytest.mark.parametrize("n,S", [(1023, 512), (1024, 512), (1025, 512), (1026, 512), (4001, 512), (4000, 511),
                                 (1, None), (2, None), (3, None)])
def test_whole_batch_sample_and_its_edges(monkeypatch, n, S):
    """n <= 2 S: the sample is the whole batch, the ranges are exact and the
    flag stays clear; above, the tail starts at an even index (odd n: the
    last op is folded on its own)."""
    if S is None:
        monkeypatch.delenv("CRDTM_PRE_SAMPLE", raising=False)
    else:
        monkeypatch.setenv("CRDTM_PRE_SAMPLE", str(S))
    ops = [(k, t, list(p), v) for k, t, p, v in _stream(n, 8, 16, 3)]
    sampled, total, exact = _tiers(_ts(ops), S or S_DEFAULT)
    assert exact == n and total == n
    assert sampled == (n > 1024)
    res, rc = _merge_and_compare(ops)
    assert rc == 0 and bool(res.flags & N.FLAG_RANGES_SAMPLED) == sampled


def _coincidence():
    """The sample's total equals n although the exact total is larger: five
    Adds of replica 200 in the middle (the sample misses them) against a range
    of replica 201 that holds five holes (its ends are in the sample)."""
    ops = _base()
    n0, k = len(ops), 5
    a = ops[10][1]
    mid = [(0, (200 << 32) + c, [a], 9) for c in range(1, k + 1)]
    ops[n0 // 2:n0 // 2] = mid
    ops.insert(100, (0, (201 << 32) + 1, [a], 9))
    ops.append((0, (201 << 32) + k + 2, [a], 9))
    return ops


def test_sample_total_equals_n_by_coincidence(monkeypatch):
    monkeypatch.setenv("CRDTM_PRE_SAMPLE", "512")
    ops = _coincidence()
    sampled, total, exact = _tiers(_ts(ops), 512)
    assert sampled and total == len(ops) and exact > len(ops)
    res, rc = _merge_and_compare(ops)  # the claim rejects replica 200's ops: the general path serves the batch
    assert rc == 0 and not res.flags & N.FLAG_RANGES_SAMPLED


def _free_index(ops, lo):
    """An op at or after `lo` that no op is anchored at and whose counter is
    not an end of its replica's range."""
    anchors = {o[2][0] for o in ops}
    ts = _ts(ops)
    rep, ctr = ts >> 32, ts & 0xFFFFFFFF
    for j in range(lo, len(ops)):
        c = ctr[rep == rep[j]]
        if ops[j][1] not in anchors and c.min() < ctr[j] < c.max():
            return j
    raise AssertionError("no such op")


@pytest.mark.parametrize("shape", ["delete", "empty_and_long_path", "negative_ts", "replica_300", "sentinel_ts",
                                   "anchor_later", "anchor_self", "duplicate_inserted", "duplicate_replacing"])
def test_failures_only_the_claim_sees(monkeypatch, shape):
    """An op in the middle of the batch, outside the sample, that the sampled
    tier must not keep: the sample still sums to n (but for the inserted
    duplicate, whose total is n - 1: the device decides), so only the claim
    and the order's checks can refuse the merge."""
    monkeypatch.setenv("CRDTM_PRE_SAMPLE", "512")
    ops = _base()
    j = _free_index(ops, len(ops) // 2)
    a, v = ops[10][1], ops[j][3]
    if shape == "delete":  # (a one-key path: n_path stays n)
        ops[j] = (1, 0, [ops[j - 1][1]], 0)
    elif shape == "empty_and_long_path":
        j2 = _free_index(ops, j + 1)
        ops[j] = (0, ops[j][1], [], v)
        ops[j2] = (0, ops[j2][1], [0, a], v)
    elif shape == "negative_ts":
        ops[j] = (0, -((3 << 32) + 5), [a], v)
    elif shape == "replica_300":
        ops[j] = (0, (300 << 32) + 1, [a], v)
    elif shape == "sentinel_ts":
        ops[j] = (0, 0, [a], v)
    elif shape == "anchor_later":
        ops[j] = (0, ops[j][1], [ops[j + 3000][1]], v)
    elif shape == "anchor_self":
        ops[j] = (0, ops[j][1], [ops[j][1]], v)
    elif shape == "duplicate_inserted":
        ops.insert(j, (0, ops[50][1], [a], v))
    elif shape == "duplicate_replacing":
        ops[j] = (0, ops[50][1], [a], v)
    sampled, total, exact = _tiers(_ts(ops), 512)
    if shape == "duplicate_inserted":
        assert not sampled and total == len(ops) - 1
    else:
        assert sampled and total == len(ops)
    res, rc = _merge_and_compare(ops, closed=shape not in ("delete", "empty_and_long_path"))
    assert not res.flags & N.FLAG_RANGES_SAMPLED


def test_timestamp_out_of_range_outside_the_sample(monkeypatch):
    """A timestamp of 2^53 + 5 in the middle: the sample does not read it, the
    claim gives it no slot, and the general path refuses the batch with
    CRDTM_E_RANGE as it always did; the tree stays fresh and merges on."""
    monkeypatch.setenv("CRDTM_PRE_SAMPLE", "512")
    ops = _base()
    j = _free_index(ops, len(ops) // 2)
    ops[j] = (0, TWO53 + 5, [ops[10][1]], ops[j][3])
    sampled, total, _ = _tiers(_ts(ops), 512)
    assert sampled and total == len(ops)
    et = CRDTree.init(0)
    with pytest.raises(N.CrdtmError):
        et.apply_arrays(_arrays(ops), len(ops))
    assert engine_summary(et) == engine_summary(CRDTree.init(0))
    res, rc = _merge_and_compare(_base(), et)
    assert rc == 0 and res.flags & N.FLAG_RANGES_SAMPLED


def test_range_edges_inside_the_sample(monkeypatch):
    monkeypatch.setenv("CRDTM_PRE_SAMPLE", "512")
    # a counter of 2^32 - 1 among the last ops: the sample sees a range far
    # beyond the slot bound, and the general path serves the batch
    ops = _base()
    r = ops[-1][1] >> 32
    ops.insert(len(ops) - 3, (0, (r << 32) + 0xFFFFFFFF, [ops[10][1]], 9))
    sampled, total, _ = _tiers(_ts(ops), 512)
    assert not sampled and total > 4 * len(ops) + 65536
    res, rc = _merge_and_compare(ops)
    assert rc == 0 and not res.flags & N.FLAG_RANGES_SAMPLED
    # the last replica id the speculation's table holds, one Add in each end
    ops = _base()
    ops.insert(7, (0, (255 << 32) + 1, [0], 9))
    ops.insert(len(ops) - 5, (0, (255 << 32) + 2, [(255 << 32) + 1], 9))
    sampled, total, exact = _tiers(_ts(ops), 512)
    assert sampled and total == exact == len(ops)
    res, rc = _merge_and_compare(ops)
    assert rc == 0 and res.flags & N.FLAG_RANGES_SAMPLED


def test_state_hygiene_on_one_tree(monkeypatch):
    """Sampled hit, sampled miss, sampled hit, then a nested batch on one tree
    handle with a reset in between: the range table and the result block's
    sample words are left clean by every exit."""
    monkeypatch.setenv("CRDTM_PRE_SAMPLE", "512")
    et = CRDTree.init(0)

    def reset():
        N.check(N.lib().crdtm_tree_reset(et._h, 0), "crdtm_tree_reset")

    res, rc = _merge_and_compare(_base(), et)
    assert rc == 0 and res.flags & N.FLAG_RANGES_SAMPLED
    reset()
    ops = _coincidence()
    assert _tiers(_ts(ops), 512)[0]
    res, rc = _merge_and_compare(ops, et)
    assert rc == 0 and not res.flags & N.FLAG_RANGES_SAMPLED
    reset()
    res, rc = _merge_and_compare(_base(), et)
    assert rc == 0 and res.flags & N.FLAG_RANGES_SAMPLED
    reset()
    s = N.synth(n_ops=8000, replicas=4, window=16, p_delete=0.2, p_branch=0.1, max_depth=3, seed=32)
    ot, rc, _ = oracle_apply_arrays(s, 8000)
    res = et.apply_arrays(s, 8000)
    assert res.code == rc == 0 and not res.flags & N.FLAG_RANGES_SAMPLED
    assert engine_summary(et) == oracle_summary(ot)
    assert np.array_equal(et.document_handles(), oracle_visible_vals(ot))
