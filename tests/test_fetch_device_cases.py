"""Pins tests/fetch_cases.py (the case table of tests/test_gpu_fetch_device.py) without a
GPU, as tests/test_geometry_helper.py pins geom.py: what the GPU tests take for granted
about their own inputs is asserted here on the CPU oracle alone."""
import os
import re

import numpy as np
import pytest

import fetch_cases as fc
import geom

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_record_sizes_cover_every_residue_mod_16():
    for tag, _, _ in fc.MATRIX_STORES:
        recs = {fc.record_bytes(c) % 16 for c in fc.CASES if c["store"] == tag}
        assert recs == {0, 4, 8, 12}, (tag, recs)
    assert {fc.record_bytes(c) for c in fc.CASES if c["dt"] == 0} == {8, 12, 16}
    assert fc.record_bytes(fc.EDGE_CASE) % 16 != 0


def test_every_store_class_width_and_key_geometry_is_present():
    for tag, vt, ada in fc.MATRIX_STORES:
        mine = [c for c in fc.CASES if c["store"] == tag]
        assert [c["cols"] for c in mine] == list(fc.WIDTHS)
        assert {c["kt"] for c in mine} == {0, 1}
        assert all(c["dt"] == 1 and c["vt"] == vt and c["ada"] == ada and c["rows"] in (301, 1237) for c in mine)
    for tag, vt, ref in fc.ARRAY_STORES:
        mine = [c for c in fc.CASES if c["store"] == tag]
        assert [c["kt"] for c in mine] == [0, 1] and all(c["dt"] == 0 and c["ref_stride"] == ref for c in mine)
    assert {c["first"] for c in fc.CASES if c["kt"] == 1} == set(fc.FIRST64)
    assert {c["first"] for c in fc.CASES if c["kt"] == 0} == set(fc.FIRST32)
    assert len({c["id"] for c in fc.CASES}) == len(fc.CASES)


def test_initial_values_hold_every_special():
    for c in fc.CASES:
        if c["cols"] < 3 and c["dt"] == 1:
            continue
        raw = fc.build_init(c).view(fc.specials(c["vt"]).dtype)
        assert set(fc.specials(c["vt"]).tolist()) <= set(raw.ravel().tolist()), c["id"]
    # the round trip's values: none that adding to zero would change
    a = fc.build_init(fc.CASES[0], plain=True)
    assert np.isfinite(a).all() and not (np.signbit(a) & (a == 0)).any()


@pytest.mark.parametrize("case", [c for c in fc.CASES if c["cols"] in (1, 5, 256)], ids=lambda c: c["id"])
def test_oracle_fetch_of_a_list_is_its_single_key_fetches(oracle, case):
    init, o = fc.make_oracle(case, oracle)
    rec = fc.record_bytes(case)
    keys = fc.key_lists(case)["shuffled"]
    assert keys.min() == case["first"] and keys.max() == case["first"] + case["rows"] - 1
    assert len(set(keys.tolist())) < len(keys)  # repeats
    whole = o.fetch(keys)
    assert len(whole) == rec * len(keys)
    sample = list(range(0, len(keys), 17)) + [len(keys) - 1]
    for i in sample:
        assert whole[i * rec:(i + 1) * rec] == o.fetch(keys[i:i + 1]), (case["id"], i)
    assert o.fetch(fc.key_lists(case)["none"]) == b""
    if case["ada"]:  # alpha varies after the push
        assert len(np.unique(o.alpha)) > 1


def test_ranges_clip_as_keyrange_intersect():
    from distml_amd.datadesc import EMPTY, KeyRange
    for c in (fc.CASES[0], fc.CASES[-1]):
        shard = KeyRange(c["first"], c["first"] + c["rows"] - 1)
        for name, (a, b, keys) in fc.ranges(c).items():
            got = shard.intersect(KeyRange(a, b))
            if len(keys) == 0:
                assert got is EMPTY, name
            else:
                assert (got.firstKey, got.lastKey) == (keys[0], keys[-1]) and got.size() == len(keys), name


def test_out_of_shard_plan_puts_the_lower_index_on_first_minus_one():
    for c in fc.CASES[::7]:
        keys, bad, reported = fc.out_of_shard_plan(c)
        first, last = c["first"], c["first"] + c["rows"] - 1
        outside = [i for i, k in enumerate(keys.tolist()) if not first <= k <= last]
        assert tuple(outside) == bad == (3, 7)
        assert keys[3] == first - 1 == reported and keys[7] == last + 1
        # the alias of test 6: inside after the reference's narrowing, outside as a 64-bit key
        alias = first + 5 + geom.ALIAS
        assert geom.row_index(alias, first, c["rows"]) == 5 and alias > last


def test_tile_constants_match_the_header_and_edges_meet_them():
    from distml_amd import _lib
    src = open(os.path.join(ROOT, "include", "distml_ps.h")).read()
    for name in ("DML_FETCH_WAVE_BYTES", "DML_FETCH_BLOCK_BYTES", "DML_KNOB_FETCH_KERNEL"):
        assert int(re.search(rf"#define {name} (\d+)", src).group(1)) == getattr(_lib, name)
    rec = fc.record_bytes(fc.EDGE_CASE)
    ns = fc.edge_counts(_lib.DML_FETCH_WAVE_BYTES, _lib.DML_FETCH_BLOCK_BYTES)
    assert len(ns) == 6 and max(ns) <= fc.EDGE_CASE["rows"]
    for unit, (a, b, c) in ((_lib.DML_FETCH_WAVE_BYTES, ns[:3]), (_lib.DML_FETCH_BLOCK_BYTES, ns[3:])):
        assert (b * rec) % unit == 0 and a == b - 1 and c == b + 1 and b * rec >= unit


def test_host_key_list_is_refused_by_name():
    """handleFetchDevice takes device keys; a host KeyList is a TypeError that names handleFetch
    (checked before the store is touched, so no GPU is needed)."""
    from distml_amd import DataDesc, DataStore, DeviceKeys, KeyList, KeyRange
    s = DataStore.__new__(DataStore)
    s.format, s.localRows, s._h, s._owned = DataDesc(1, 0, 1), KeyRange(0, 9), None, False
    with pytest.raises(TypeError, match="handleFetch"):
        s.handleFetchDevice(s.format, KeyList([1, 2]), 0, 0)
    assert DeviceKeys(256, 3).n == 3
