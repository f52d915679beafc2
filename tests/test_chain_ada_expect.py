"""CPU: the AdaGrad chain's yardstick (tests/chain_ada_expect.py) can tell, on the very
inputs the GPU tests use (test_gpu_chain_ada.py, test_native_chain_ada.py):

  - the rank-major order gives other delta bits than the ring order;
  - after every call between 20 % and 80 % of the elements have delta > 1, so alpha both
    moves and stays;
  - the maxDelta tie inputs give the stated holder under the ring order and another one
    under rank-major;
  - the setAlpha case has rows call 1 does not list whose delta is above 1 (they must keep
    the set alpha) and a listed row of zero gradients with delta above 1 (recomputed);
  - the NaN case leaves exactly its two named elements out of the alpha comparison.
"""
import numpy as np
import pytest

import chain_ada_expect as A
import chain_expect as X


def share_above_one(state):
    d = np.concatenate([sh["delta"].ravel() for sh in state])
    return float((d > 1.0).mean())


@pytest.mark.parametrize("world,rows,cols,pieces,asc,blocked", A.RING_CASES)
def test_ring_inputs_discriminate(oracle, world, rows, cols, pieces, asc, blocked):
    calls = A.ring_calls(world, rows, cols, asc)
    init = X.init_values(A.VT, rows, cols)
    ring = A.expected(oracle, world, rows, cols, calls, init)
    major = A.expected(oracle, world, rows, cols, calls, init, order=X.rank_major)
    for c in range(A.RING_CALLS):
        share = share_above_one(ring[c])
        print(f"{world} x {rows} x {cols} call {c}: share of delta > 1 = {share:.3f}")
        assert 0.20 <= share <= 0.80, (c, share)
    last = A.RING_CALLS - 1
    assert X.same_bits(ring[last][0]["delta"], major[last][0]["delta"], A.VT)  # shard 0: the same order
    for s in range(1, world):
        diff = X.bits(ring[last][s]["delta"], A.VT) != X.bits(major[last][s]["delta"], A.VT)
        print(f"  shard {s}: {int(diff.sum())} of {diff.size} delta bits differ")
        assert diff.mean() >= 0.05, (s, diff.mean())


@pytest.mark.parametrize("asc", [False, True])
@pytest.mark.parametrize("case", ["a", "b", "c"])
def test_tie_inputs_name_their_holder(oracle, case, asc):
    calls, ring_holder, major_holder = A.tie_calls(case, asc)
    init = X.init_values(A.VT, A.TIE_ROWS, A.TIE_COLS)
    ring = A.expected(oracle, A.TIE_WORLD, A.TIE_ROWS, A.TIE_COLS, calls, init)
    major = A.expected(oracle, A.TIE_WORLD, A.TIE_ROWS, A.TIE_COLS, calls, init, order=X.rank_major)
    for c in range(len(calls)):
        assert ring[c][1]["md"] == (4.0, ring_holder[0], ring_holder[1]), ring[c][1]["md"]
        assert major[c][1]["md"] == (4.0, major_holder[0], major_holder[1]), major[c][1]["md"]
        assert ring[c][0]["md"][0] < 1e-3  # shard 0: small gradients only
    assert ring_holder != major_holder
    # more than one element holds the maximum: a tie indeed
    assert int((ring[-1][1]["delta"] == 4.0).sum()) >= 2


def test_set_alpha_inputs_have_the_rows_that_matter(oracle):
    world, W, rows, cols = 2, 5, 300, 64
    calls = A.set_alpha_calls(world, W, rows, cols)
    init = X.init_values(A.VT, rows, cols)
    want = A.expected(oracle, world, rows, cols, calls, init, set_alpha={0: A.SET_ALPHA})
    unlisted = np.arange(5, rows, 7)
    kept = recomputed = 0
    for s, (f, l) in enumerate(X.shard_ranges(world, rows)):
        un = unlisted[(unlisted >= f) & (unlisted <= l)] - f
        above = want[1][s]["delta"][un] > 1.0
        kept += int(above.sum())
        # unlisted rows: every alpha is the set value, also where delta > 1
        assert (want[1][s]["alpha"][un] == np.float32(A.SET_ALPHA[0])).all()
        if f <= A.ZERO_ROW <= l:
            z = A.ZERO_ROW - f
            hot = want[1][s]["delta"][z] > 1.0
            recomputed += int(hot.sum())
            assert (want[1][s]["alpha"][z][hot] != np.float32(A.SET_ALPHA[0])).all()
            assert X.same_bits(want[1][s]["delta"][z], want[0][s]["delta"][z], A.VT)  # zero gradients
    assert kept > 0 and recomputed > 0, (kept, recomputed)
    assert 0.20 <= share_above_one(want[0]) <= 0.80 and 0.20 <= share_above_one(want[1]) <= 0.80


def test_special_inputs_name_their_elements(oracle):
    world, W, rows, cols = 3, 5, 300, 64
    calls, inf_el, nan_els = A.special_calls(world, W, rows, cols)
    init = X.minus_zero_init(A.VT, rows, cols)
    want = A.expected(oracle, world, rows, cols, calls, init)
    rng = X.shard_ranges(world, rows)
    shard_of = lambda row: next(s for s, (f, l) in enumerate(rng) if f <= row <= l)  # noqa: E731
    assert shard_of(nan_els[0][0]) != shard_of(nan_els[1][0])
    masked = {(f + int(r), int(c)) for s, (f, l) in enumerate(rng)
              for r, c in zip(*np.nonzero(A.nan_alpha_mask(want[1][s]["delta"])))}
    assert masked == set(nan_els), (masked, nan_els)
    assert not any(A.nan_alpha_mask(want[0][s]["delta"]).any() for s in range(world))
    # the alpha they held before the call was a computed one, and the reference moved it on
    for (row, col) in nan_els:
        s = shard_of(row)
        assert want[0][s]["delta"][row - rng[s][0], col] > 1.0
    s = shard_of(inf_el[0])
    assert np.isposinf(want[0][s]["delta"][inf_el[0] - rng[s][0], inf_el[1]])
    assert want[1][s]["md"] == (np.inf, inf_el[0], inf_el[1])
    for c in range(2):
        assert 0.20 <= share_above_one(want[c]) <= 0.80


def test_bindings_exist():
    from distml_amd import _lib
    from distml_amd.group import HipOps
    assert "dml_prereduce_chain_piece_ada" in _lib.SIGNATURES and "dml_store_assign_adagrad_device" in _lib.SIGNATURES
    assert hasattr(HipOps, "chain_piece_ada") and hasattr(HipOps, "assign_ada")
