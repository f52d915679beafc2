"""The sequence generator (tests/opseq.py) against the CPU oracle alone.

tests/test_gpu_opseq.py trusts a sequence's plan: which calls fail, with which
(code, key, col), and which paths the applied calls reach. Everything about that plan
that does not need the GPU is checked here, for every (config, seed) the GPU test uses.
"""
import functools

import numpy as np
import pytest

import opseq


@functools.lru_cache(maxsize=None)
def _run(name, seed):
    """One sequence through the oracle only; a summary without the big arrays."""
    import pyoracle
    pyoracle.build()
    cfg = opseq.CONFIGS[name]
    seq = opseq.make_sequence(name, seed)
    side = opseq.OracleSide(pyoracle, cfg, seq[0])
    init = seq[0]["values"].copy()
    bursts = opseq.bursts_of(seq)
    got_errors, planned_errors, shape = [], [], []
    for bi, (calls, sync) in enumerate(bursts):
        err = None
        for ci, call in enumerate(calls):
            if call["applied"]:
                assert err is None, "an applied call behind the burst's error"
                e = side.push_call(call)
                if e is not None:
                    err = e
                    got_errors.append((bi, ci, e))
            if call["error"] is not None:
                planned_errors.append((bi, ci, tuple(call["error"])))
        side.clear_error()
        side.sync(sync)
        assert side.o.error()[0] == 0
        shape.append(([(c["kind"], len(c["pushes"]), c["applied"], c["error"] is not None) for c in calls],
                      sync["kind"], sync["end"]))
    udt = opseq.UDT[cfg["value_type"]]
    changed = (side.o.data.view(udt) != init.view(udt)).any(axis=1).sum()
    return dict(digest=opseq.digest(seq), nops=len(seq) - 1, got=got_errors, planned=planned_errors, shape=shape,
                changed=int(changed), expects=opseq.expected_paths(seq))


@pytest.mark.parametrize("name,seed", opseq.CASES)
def test_sequence_plan_holds_on_the_oracle(name, seed):
    cfg = opseq.CONFIGS[name]
    r = _run(name, seed)
    # the same seed gives the same bytes
    assert opseq.digest(opseq.make_sequence(name, seed)) == r["digest"]
    # the oracle fails at exactly the planned calls with exactly the planned (code, key, col)
    assert r["got"] == r["planned"], (r["got"], r["planned"])
    # shape: 20-30 ops, bursts of 1-4 calls with at most one error, calls of 1-9 pushes plus
    # one of 65-70 on the narrow configs only
    assert 20 <= r["nops"] <= 30, r["nops"]
    long_calls = 0
    for calls, _, _ in r["shape"]:
        assert 1 <= len(calls) <= 4
        assert sum(1 for c in calls if c[3]) <= 1
        for kind, nb, applied, _ in calls:
            if kind == "long":
                assert 65 <= nb <= 70 and not cfg["wide"]
                long_calls += 1
            else:
                assert 1 <= nb <= 9, (kind, nb)
    assert long_calls == (0 if cfg["wide"] else 1)
    ends = [e for _, _, e in r["shape"]]
    assert "retire" in ends and "drop" in ends
    # at least a third of the bursts hold no error: pipelined success paths run
    clean = sum(1 for calls, _, _ in r["shape"] if not any(c[3] for c in calls))
    assert 3 * clean >= len(r["shape"]), (clean, len(r["shape"]))
    # the sequence recovers from its errors: the shard ends far from where it began
    assert 2 * r["changed"] >= cfg["rows"], r["changed"]
    # the paths the GPU test asserts are planned in every sequence, so no assertion there is vacuous
    want = set()
    if opseq.spec_shaped(cfg):
        want |= {"spec", "rerun", "reuse", "identity"}
        if opseq.flat_shaped(cfg):
            want.add("ident_launch")
    if cfg["ada"] and opseq.flat_shaped(cfg):
        want |= {"k_ada_ident", "k_ada_flat"}
    if cfg["data_type"] == opseq.ARRAY:
        want.add("sparse_skew")
    assert want <= set(r["expects"]), (want, r["expects"])


@pytest.mark.parametrize("name", list(opseq.CONFIGS))
def test_every_op_kind_occurs_over_the_seeds(name):
    cfg = opseq.CONFIGS[name]
    pushes, syncs = set(), set()
    for seed in opseq.SEEDS:
        for calls, sync_kind, _ in _run(name, seed)["shape"]:
            pushes |= {kind for kind, _, applied, _ in calls if applied}
            syncs.add(sync_kind)
    assert pushes == set(opseq.push_kinds(cfg)), set(opseq.push_kinds(cfg)) ^ pushes
    assert syncs == set(opseq.sync_kinds(cfg)), set(opseq.sync_kinds(cfg)) ^ syncs


def test_planned_corruptions_hide_from_the_identity_sample():
    """The swapped / repeated records sit where k_ident_check does not look (its sample is
    restated in opseq.sampled_positions), so speculation meets them in the reduce."""
    for name in ("f32_c1024", "f32_c200", "f64_c100"):
        cfg = opseq.CONFIGS[name]
        R, stride = cfg["rows"], opseq.record_stride(cfg)
        kdt = opseq._kdt(cfg)
        for op in opseq.make_sequence(name, 1):
            if op["op"] != "push" or op["kind"] not in ("swap", "dup"):
                continue
            moved = 0
            for b, p in enumerate(op["pushes"]):
                keys = p.reshape(R, stride)[:, :kdt.itemsize].copy().view(kdt).ravel() - cfg["first"]
                off = np.nonzero(keys != np.arange(R))[0]
                if 0 < len(off) <= 2:  # an ascending push with one corruption
                    moved += 1
                    assert not set(off.tolist()) & opseq.sampled_positions(b, R)
            assert moved >= 1 or op["kind"] == "dup"  # (a repeat may sit in a permuted push)


def test_splitmix64_matches_the_oracle(oracle):
    for x in (0, 1, (5 << 32) + 40, (1 << 64) - 1):
        assert opseq.splitmix64(x) == oracle.splitmix64(x)
