"""The two ways out of the radix-partitioned aggregate (capi.cpp run_radix) when its LDS buckets or its result do not hold the groups:
forced with strategy "radix" the caller's too-small hint is a capacity error; reached by strategy "auto" the run goes on through the
global hash table and gives the same groups.  Expected values by numpy (where every key is distinct, each group is its own row)."""
import numpy as np
import pyarrow as pa
import pytest

import arrow_ballista_amd as g
from arrow_ballista_amd.expr import col, lit

pytestmark = pytest.mark.gpu


def distinct_keys_plan(n, seed, domain=None, **kw):
    """n rows keyed by a UInt32 column: all keys distinct, or drawn from `domain` values"""
    r = np.random.default_rng(seed)
    keys = ((r.permutation(n) if domain is None else r.integers(0, domain, n)).astype(np.int64) * 3 + 1).astype(np.uint32)
    v = r.integers(-10**9, 10**9, n)
    src = g.MemoryExec([pa.table({"u32": pa.array(keys), "v": pa.array(v)})])
    s = src.schema()
    aggs = [{"fn": "COUNT", "expr": lit(1), "name": "c"}, {"fn": "SUM", "expr": col("v", s), "name": "sv"}]
    return g.AggregateExec("Single", [(col("u32", s), "u32")], aggs, src, **kw), keys, v


def test_radix_with_a_too_small_hint_is_a_capacity_error(tc):
    """expected_groups = 1 gives one bucket; 5000 distinct keys are more than any LDS table holds (at most 1024 slots of this shape)."""
    plan, _, _ = distinct_keys_plan(5000, 1, strategy="radix", expected_groups=1)
    with pytest.raises(g.GpuqError) as e:
        plan.execute(0, tc)
    assert e.value.status == 4 and "bucket overflowed" in str(e.value)


def test_auto_leaves_an_overflowing_radix_run_for_the_global_table(tc):
    """2^20 + 4097 distinct keys with a hint of 800,000 groups: "auto" takes the radix path (>= 2^20 rows, >= 4096 groups known), whose
    result is laid out for max(hint + 1/4, 2^20) = 2^20 groups -- fewer than there are.  The run must finish through the global table
    (sized from the hint: 2^21 slots hold the keys without growing; then counted and extracted) with every group."""
    n = (1 << 20) + 4097
    plan, keys, v = distinct_keys_plan(n, 2, expected_groups=800_000)
    t = g.NativePlan(plan, tc).execute(0).to_arrow()
    got_k = t["u32"].to_numpy()
    order = np.argsort(got_k)
    want = np.argsort(keys)
    assert len(got_k) == n and np.array_equal(got_k[order], keys[want])
    assert np.array_equal(t["c"].to_numpy()[order], np.ones(n, dtype=np.int64))
    assert np.array_equal(t["sv"].to_numpy()[order], v[want])


def test_auto_radix_run_that_holds(tc):
    """the same shape with 300,000 possible keys and the hint to match: the radix run "auto" chooses holds all groups and is the result"""
    n = (1 << 20) + 4097
    plan, keys, v = distinct_keys_plan(n, 3, domain=300_000, expected_groups=300_000)
    t = g.NativePlan(plan, tc).execute(0).to_arrow()
    u, inv = np.unique(keys, return_inverse=True)
    sv = np.zeros(len(u), dtype=np.int64)
    np.add.at(sv, inv, v)
    order = np.argsort(t["u32"].to_numpy())
    assert np.array_equal(t["u32"].to_numpy()[order], u)
    assert np.array_equal(t["c"].to_numpy()[order], np.bincount(inv))
    assert np.array_equal(t["sv"].to_numpy()[order], sv)
