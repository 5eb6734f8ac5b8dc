"""CPU: which aggregate keys the compile finds small enough for the hash table's state word (csrc/agg_compile.cpp, KeySpec::state_key):
the whole key, one NULL flag per nullable column included, in at most 62 bits of narrow integer / date columns."""
import arrow_ballista_amd as g
from arrow_ballista_amd.expr import col

FIELDS = [{"name": "u32", "type": "UInt32", "nullable": False}, {"name": "i32n", "type": "Int32", "nullable": True}, {"name": "d", "type": "Date32", "nullable": False},
          {"name": "dn", "type": "Date32", "nullable": True}, {"name": "i16n", "type": "Int16", "nullable": True}, {"name": "i8n", "type": "Int8", "nullable": True},
          {"name": "i64", "type": "Int64", "nullable": False}, {"name": "s", "type": "Utf8", "nullable": False}, {"name": "dec", "type": {"Decimal128": [15, 2]}, "nullable": False},
          {"name": "v", "type": "Int64", "nullable": True}]


def state_key(groups):
    d = {"op": "aggregate", "mode": "Single", "input": {"fields": FIELDS}, "strategy": "hash", "group_expr": [{"expr": col(n, FIELDS), "name": n} for n in groups],
         "aggr_expr": [{"fn": "SUM", "expr": col("v", FIELDS), "name": "sv"}]}
    return g.compile_check(d)["state_key"]


def test_keys_that_fit_the_state_word():
    for groups in (["u32"], ["i32n"], ["d"], ["dn"], ["i16n", "i8n"], ["i8n", "i16n", "i32n"], ["u32", "i16n", "i8n"]):      # 32, 33, 32, 33, 26, 59, 58 bits
        assert state_key(groups) is True, groups


def test_keys_that_do_not():
    for groups in (["i64"], ["s"], ["dec"], ["u32", "i32n"], ["i64", "d", "i32n"], ["d", "dn"], []):      # 64 bits, strings, 128 bits, 65, >62, 65, no key
        assert state_key(groups) is False, groups
