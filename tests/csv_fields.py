"""Hand-built delimited text for the device text decoder (csrc/kernels_scanfmt.hip: k_csv_count_lines, k_csv_line_starts,
k_csv_parse, k_csv_copy_strings; csrc/scanfmt.cpp: gpuq_csv_decode; scan.read_csv).

A writer emits only well-formed fields.  A per-field parser that accepts a bad one does not crash: it puts a plausible wrong value
into a column.  The corpus here is one field per case -- at the bounds of every type, in every spelling the grammar allows and
one step outside it -- and whole files, the smallest that reach a boundary of the line splitter (the 64-row ballot words, the
256-line block, the 64 KiB line-split chunk, the 40 KiB LDS staging budget).

A field case is (name, column type, nullable, field bytes, expect).  `expect` is a value, NULL or a Refused(status, word of the
message).  The values come from plain Python, not from the code under test and not from pyarrow: int(text), decimal.Decimal scaled
to an int, float(text) (correctly rounded; compared bit for bit), datetime.date.fromisoformat(text).  Every comparison is exact.

Status 1 is malformed text.  Status 3 is text the device does not decode although it is well-formed for a reader: a quoted field,
a Float64 outside the exact fast path (Refused.value then holds float(text), and a host reader must agree with it), a blank line, a
carriage return that does not precede a line feed.  reference_field() / reference_file() state the grammar the device enforces,
independently of the case list; test_cpu_csv_fields.py holds the two against each other and against pyarrow.  Plain Python: nothing
here touches the GPU or imports the project.
"""
import datetime
import decimal
import functools
import re
import struct
from collections import namedtuple

Case = namedtuple("Case", "name ctype nullable field expect")
Layout = namedtuple("Layout", "name schema text delimiter header projection expect pyarrow")      # expect: "rows" or a Refused


class _Null:
    def __repr__(self):
        return "NULL"


NULL = _Null()


class Refused(Exception):
    def __init__(self, status, word, value=None):
        Exception.__init__(self, "refused(%d, %r)" % (status, word))
        self.status, self.word, self.value = status, word, value

    def __eq__(self, other):
        return isinstance(other, Refused) and (self.status, self.word) == (other.status, other.word)

    def __hash__(self):
        return hash((self.status, self.word))


def refused(status, word, value=None):
    return Refused(status, word, value)


PARSE, REQUIRED, COUNT = (1, "parse"), (1, "non-nullable"), (1, "number of fields")
FAST_PATH, QUOTED, BLANK, BARE_CR = (3, "Float64"), (3, "quoted"), (3, "blank line"), (3, "carriage return")

EPOCH = datetime.date(1970, 1, 1).toordinal()
DEC_PAIRS = [(5, 2), (15, 2), (38, 0), (38, 10), (38, 38)]
BOOL_SPELLINGS = {b"true": True, b"True": True, b"TRUE": True, b"false": False, b"False": False, b"FALSE": False}


def dec(p, s):
    return {"Decimal128": [p, s]}


def type_key(ctype):
    return "Decimal128(%d,%d)" % tuple(ctype["Decimal128"]) if isinstance(ctype, dict) else ctype


def float_bits(v):
    return struct.unpack("<Q", struct.pack("<d", v))[0]


# ---------------------------------------------------------------- the grammar the device enforces, stated once in plain Python
_INT = re.compile(rb"[+-]?[0-9]+\Z")
_DEC = re.compile(rb"[+-]?(?:([0-9]+)(?:\.([0-9]*))?|\.([0-9]+))\Z")
_FLT = re.compile(rb"([+-]?)(?:([0-9]+)(?:\.([0-9]*))?|\.([0-9]+))(?:[eE]([+-]?[0-9]+))?\Z")
_DATE = re.compile(rb"[0-9]{4}-[0-9]{2}-[0-9]{2}\Z")


def reference_field(ctype, nullable, field):
    """the value of one field, NULL, or raise Refused.  (The lexical checks of a whole line -- quote, carriage return -- are
    reference_file's.)"""
    if ctype == "Utf8":
        return NULL if (field == b"" and nullable) else field.decode()
    if field == b"":
        if nullable:
            return NULL
        raise refused(*REQUIRED)
    if ctype in ("Int32", "Int64"):
        if not _INT.match(field):
            raise refused(*PARSE)
        v, bits = int(field), 31 if ctype == "Int32" else 63
        if not -(1 << bits) <= v < (1 << bits):
            raise refused(*PARSE)
        return v
    if ctype == "Date32":
        if not _DATE.match(field):
            raise refused(*PARSE)
        try:
            return datetime.date.fromisoformat(field.decode()).toordinal() - EPOCH      # (year 0000 is no date of datetime's: refused)
        except ValueError:
            raise refused(*PARSE)
    if ctype == "Boolean":
        if field not in BOOL_SPELLINGS:
            raise refused(*PARSE)
        return BOOL_SPELLINGS[field]
    if ctype == "Float64":
        m = _FLT.match(field)
        if not m:
            raise refused(*PARSE)
        value = float(field)
        digits = ((m.group(2) or b"") + (m.group(3) or b"") + (m.group(4) or b"")).lstrip(b"0")
        n_frac = len(m.group(3) or m.group(4) or b"")
        if digits == b"":
            return -0.0 if m.group(1) == b"-" else 0.0
        # Clinger's fast path: the digits (trailing zeros included, as written) form an integer w < 2^53 of at most 19 digits and
        # the decimal exponent left after the fraction digits lies in -22..22: one correctly rounded multiply or divide
        e10 = int(m.group(5) or b"0") - n_frac
        if len(digits) > 19 or int(digits) >= 1 << 53 or not -22 <= e10 <= 22:
            raise refused(*FAST_PATH, value=value)
        return value
    p, s = ctype["Decimal128"]
    m = _DEC.match(field)
    if not m:
        raise refused(*PARSE)
    if len(m.group(2) or m.group(3) or b"") > s:
        raise refused(*PARSE)      # more fraction digits than the column's scale: refused, never rounded
    v = unscaled(decimal.Decimal(field.decode()), s)
    if abs(v) >= 10 ** p:
        raise refused(*PARSE)
    return v


def reference_file(text, schema, delimiter=b",", header=False, projection=None):
    """{column name: [values]} of the projected columns, or raise Refused: the text split into lines at every line feed (one
    carriage return before it belongs to the line end; the last line may go without), every line into fields at the delimiter
    (a delimiter after the last field is allowed), every projected field through reference_field.  Refusals in the order the
    decoder reports them."""
    lines = text.split(b"\n")
    if lines[-1] == b"":
        lines.pop()
    lines = [ln[:-1] if ln.endswith(b"\r") else ln for ln in lines][1 if header else 0:]
    names = [s[0] for s in schema]
    keep = list(range(len(schema))) if projection is None else [names.index(p) if isinstance(p, str) else p for p in projection]
    rows = []
    found = set()
    for ln in lines:
        if b'"' in ln:
            found.add(Refused(*QUOTED))
        if b"\r" in ln:
            found.add(Refused(*BARE_CR))
        if ln == b"":
            found.add(Refused(*BLANK))
            continue
        pieces = ln.split(delimiter)
        if len(pieces) == len(schema) + 1 and pieces[-1] == b"":
            pieces.pop()
        if len(pieces) != len(schema):
            found.add(Refused(*COUNT))
            continue
        row = []
        for i in keep:
            try:
                row.append(reference_field(schema[i][1], schema[i][2], pieces[i]))
            except Refused as e:
                found.add(Refused(e.status, e.word))
                row.append(None)
        rows.append(row)
    for r in (QUOTED, BARE_CR, BLANK, COUNT, PARSE, REQUIRED, FAST_PATH):
        if Refused(*r) in found:
            raise refused(*r)
    return {names[i]: [row[k] for row in rows] for k, i in enumerate(keep)}


# ---------------------------------------------------------------- field cases
def _int_cases():
    out = []
    for ty, bits in (("Int32", 31), ("Int64", 63)):
        hi, lo = (1 << bits) - 1, -(1 << bits)

        def ok(name, text, ty=ty):
            out.append(Case("%s/%s" % (ty.lower(), name), ty, False, text.encode(), int(text)))

        def bad(name, field, ty=ty, why=PARSE, nullable=False):
            out.append(Case("%s/refused_%s" % (ty.lower(), name), ty, nullable, field, refused(*why)))
        ok("max", str(hi)); ok("min", str(lo)); ok("max_plus_sign", "+%d" % hi); ok("zero", "0"); ok("minus_zero", "-0"); ok("plus_five", "+5")
        ok("leading_zeros", "007"); ok("41_zeros_then_7", "0" * 41 + "7"); ok("minus_leading_zeros", "-00012"); ok("zeros_then_max", "0" * 30 + str(hi))
        ok("one", "1"); ok("minus_one", "-1")
        bad("max_plus_1", str(hi + 1).encode()); bad("min_minus_1", str(lo - 1).encode()); bad("ten_times_max", str(hi * 10).encode())
        bad("2_pow_64", b"18446744073709551616"); bad("2_pow_64_plus_1", b"18446744073709551617"); bad("thirty_digits", b"1" * 30)
        bad("lone_minus", b"-"); bad("lone_plus", b"+"); bad("two_signs", b"--1"); bad("inner_sign", b"1-2"); bad("trailing_sign", b"12-")
        bad("leading_space", b" 1"); bad("trailing_space", b"1 "); bad("fraction", b"1.0"); bad("exponent", b"1e2"); bad("hex", b"0x10")
        bad("slash_below_0", b"1/"); bad("colon_above_9", b"1:"); bad("arabic_indic_digit", "١".encode()); bad("letters", b"abc")
        bad("empty_required", b"", why=REQUIRED)
        out.append(Case("%s/empty_nullable" % ty.lower(), ty, True, b"", NULL))
        out.append(Case("%s/value_in_nullable" % ty.lower(), ty, True, b"-42", -42))
        bad("lone_minus_nullable", b"-", nullable=True)
    return out


def _date_cases():
    out = []
    for text in ("0001-01-01", "1969-12-31", "1970-01-01", "1970-01-02", "2024-02-29", "2000-02-29", "9999-12-31", "1600-02-29", "2023-12-31",
                 "2023-01-31", "2023-03-31", "2023-04-30", "2023-05-31", "2023-06-30", "2023-07-31", "2023-08-31", "2023-09-30", "2023-10-31", "2023-11-30",
                 "2023-02-28", "1900-02-28", "1900-03-01", "0004-02-29"):
        out.append(Case("date32/" + text, "Date32", False, text.encode(), datetime.date.fromisoformat(text).toordinal() - EPOCH))
    bad = [("feb_29_of_2023", b"2023-02-29"), ("feb_29_of_1900", b"1900-02-29"), ("feb_29_of_2100", b"2100-02-29"), ("feb_30", b"2023-02-30"), ("month_00", b"2023-00-10"),
           ("month_13", b"2023-13-01"), ("month_13_day_45", b"2023-13-45"), ("day_00", b"2023-01-00"), ("day_32", b"2023-01-32"), ("apr_31", b"2023-04-31"),
           ("jun_31", b"2023-06-31"), ("sep_31", b"2023-09-31"), ("nov_31", b"2023-11-31"), ("day_99", b"2023-12-99"), ("month_99", b"2023-99-01"),
           ("letters", b"abcd-ef-gh"), ("slashes", b"2023/01/01"), ("nine_bytes", b"2023-1-15"), ("nine_bytes_short_year", b"023-01-15"),
           ("eleven_bytes", b"2023-01-015"), ("eleven_bytes_long_year", b"12023-01-15"), ("no_dashes", b"20230115"), ("year_0000", b"0000-01-01"),
           ("dash_for_a_digit", b"2023-01--1"), ("time_attached", b"2023-01-15T00:00:00"), ("trailing_space", b"2023-01-15 ")]
    for at in (0, 1, 2, 3, 5, 6, 8, 9):      # a non-digit in each of the eight digit positions: a letter, and the bytes just outside '0'..'9'
        for ch, what in ((b"x", "letter"), (b"/", "slash"), (b":", "colon"), (b" ", "space")):
            f = bytearray(b"2023-01-15")
            f[at:at + 1] = ch
            bad.append(("%s_at_%d" % (what, at), bytes(f)))
    for name, f in bad:
        out.append(Case("date32/refused_" + name, "Date32", False, f, refused(*PARSE)))
    out.append(Case("date32/refused_empty_required", "Date32", False, b"", refused(*REQUIRED)))
    out.append(Case("date32/empty_nullable", "Date32", True, b"", NULL))
    out.append(Case("date32/value_in_nullable", "Date32", True, b"1999-12-31", datetime.date(1999, 12, 31).toordinal() - EPOCH))
    return out


def unscaled(d, s):
    """a decimal.Decimal as the integer a Decimal128 column of scale s stores: exact, whatever the context's precision"""
    sign, digits, exp = d.as_tuple()
    assert exp + s >= 0
    v = int("".join(map(str, digits))) * 10 ** (exp + s)
    return -v if sign else v


def _scaled(text, s):
    return unscaled(decimal.Decimal(text), s)


def _dec_cases():
    out = []
    for p, s in DEC_PAIRS:
        ty, tag = dec(p, s), "decimal_%d_%d" % (p, s)
        ni = p - s      # integer digits

        def ok(name, text, ty=ty, tag=tag, s=s):
            out.append(Case("%s/%s" % (tag, name), ty, False, text.encode(), _scaled(text, s)))

        def bad(name, field, ty=ty, tag=tag, why=PARSE, nullable=False):
            out.append(Case("%s/refused_%s" % (tag, name), ty, nullable, field if isinstance(field, bytes) else field.encode(), refused(*why)))
        big = ("9" * ni if ni else "0") + ("." + "9" * s if s else "")
        ok("zero", "0"); ok("largest", big); ok("smallest", "-" + big); ok("largest_plus_sign", "+" + big); ok("integer_dot", "0." if ni == 0 else "1.")
        ok("zeros_then_largest", "0" * 45 + big)
        if ni:
            ok("one", "1"); ok("minus_one", "-1"); ok("plus_five", "+5"); ok("leading_zeros", "007"); ok("integer_nines", "9" * ni)
        if s:
            ok("dot_five", ".5"); ok("minus_dot_five", "-.5"); ok("one_fraction_digit", "0.7"); ok("full_fraction", "0." + "0" * (s - 1) + "1")
            ok("largest_without_integer_part", "." + "9" * s)
        if s >= 2:
            ok("two_fraction_digits", "0.25"); ok("minus_zero", "-0.00"); ok("zero_fraction", "0.00")
        else:
            ok("minus_zero", "-0")
        if ni and s >= 2:
            ok("1_5", "1.5"); ok("1_50", "1.50"); ok("minus_12_34", "-12.34" if ni >= 2 else "-2.34")
        # one digit beyond the precision: written out, and reached only by the zeros the scale appends
        beyond = "1" + "0" * ni
        bad("one_digit_beyond", beyond + ("." + "0" * s if s else "")); bad("minus_one_digit_beyond", "-" + beyond + ("." + "0" * s if s else ""))
        if s:
            bad("one_digit_beyond_by_scale_padding", beyond); bad("nines_beyond_by_scale_padding", "9" * (ni + 1))
        bad("fraction_longer_than_scale", "0." + "0" * s + "1"); bad("zero_fraction_longer_than_scale", "1." + "0" * (s + 1) if ni else "0." + "0" * (s + 1))
        bad("two_dots", "1.2.3"); bad("dots_only", ".."); bad("exponent", "1e2"); bad("inner_sign", "1-2"); bad("leading_space", " 1"); bad("trailing_space", "1 ")
        bad("lone_minus", "-"); bad("lone_plus", "+"); bad("lone_dot", "."); bad("minus_dot", "-."); bad("plus_dot", "+."); bad("letters", "abc")
        bad("slash_below_0", "1/"); bad("colon_above_9", "1:"); bad("empty_required", "", why=REQUIRED)
        bad("lone_dot_nullable", ".", nullable=True)
        out.append(Case(tag + "/empty_nullable", ty, True, b"", NULL))
        # fields a 128-bit accumulator wraps on: every one has more than 38 digits (or reaches them with the scale's zeros)
        for name, v in (("2_pow_127", 1 << 127), ("2_pow_128", 1 << 128), ("2_pow_128_plus_5", (1 << 128) + 5), ("2_pow_128_plus_1_negative", -((1 << 128) + 1)),
                        ("39_nines", 10 ** 39 - 1), ("40_nines", 10 ** 40 - 1), ("41_digits", 3 * (1 << 128) * 10 + 7), ("60_digits", 10 ** 59 + 1),
                        ("2_pow_127_plus_9", (1 << 127) + 9)):
            bad("wrap_" + name, str(v))
        if s:
            # the smallest integer whose padding by 10^s passes a multiple of 2^128: it wraps to a small positive remainder
            for k in (1, 2, 3):
                x = -(-(k << 128) // 10 ** s)
                bad("wrap_by_scale_padding_%d" % k, str(x))
    bad_3810 = [("thirty_digits_into_scale_10", "1" + "0" * 29), ("thirty_nines_into_scale_10", "9" * 30), ("29_digits_into_scale_10", "1" + "0" * 28),
                ("39_digits_with_fraction", "1" + "0" * 28 + "." + "0" * 10)]
    for name, f in bad_3810:
        out.append(Case("decimal_38_10/refused_" + name, dec(38, 10), False, f.encode(), refused(*PARSE)))
    out.append(Case("decimal_15_2/value_in_nullable", dec(15, 2), True, b"-1234567890123.45", -123456789012345))
    return out


def _float_cases():
    out = []

    def ok(name, text):
        out.append(Case("float64/" + name, "Float64", False, text.encode(), float(text)))

    def slow(name, text):      # well-formed, outside the exact fast path: refused with status 3, never rounded differently
        out.append(Case("float64/outside_fast_path_" + name, "Float64", False, text.encode(), refused(*FAST_PATH, value=float(text))))

    def bad(name, field, why=PARSE, nullable=False):
        out.append(Case("float64/refused_" + name, "Float64", nullable, field, refused(*why)))
    ok("zero", "0"); ok("one", "1"); ok("minus_one", "-1"); ok("plus_one", "+1"); ok("2_pow_53_minus_1", str((1 << 53) - 1)); ok("minus_2_pow_53_minus_1", "-" + str((1 << 53) - 1))
    ok("e22", "1e22"); ok("e_minus_22", "1e-22"); ok("capital_e", "1E22"); ok("e_plus_5", "1e+5"); ok("capital_e_minus_5", "1E-5"); ok("dot_five", ".5"); ok("five_dot", "5.")
    ok("minus_dot_five", "-.5"); ok("minus_zero_dot_zero", "-0.0"); ok("minus_zero", "-0"); ok("plus_zero", "+0"); ok("zero_e999", "0e999"); ok("minus_zero_e999", "-0e999")
    ok("zero_e_minus_999", "0e-999"); ok("zero_with_exponent_2_pow_32", "0.0e4294967296"); ok("zero_dot_30_zeros", "0." + "0" * 30); ok("dot_e", "5.e3"); ok("dot_five_e", ".5e1")
    ok("leading_zeros", "0001.5"); ok("45_leading_zeros", "0" * 45 + "2.5"); ok("zeros_after_dot", "1.0005"); ok("small_fraction", "0.001"); ok("all_zeros", "000.000")
    ok("15_digits", "123456789012345"); ok("16_digits_below_2_pow_53", "1234567890123456"); ok("15_digits_fraction_e7", "1.23456789012345e7")
    ok("15_digits_e_minus_22", "123456789012345e-22"); ok("15_digits_e22", "123456789012345e22"); ok("1e_minus_22_written_out", "0." + "0" * 21 + "1")
    ok("15e22", "15e22"); ok("1_5e23", "1.5e23"); ok("fraction_moves_exponent_into_range", "0.001e25"); ok("2_pow_53_minus_1_e22", str((1 << 53) - 1) + "e22")
    ok("2_pow_53_minus_1_e_minus_22", str((1 << 53) - 1) + "e-22"); ok("trailing_zeros", "1.5000"); ok("point_one", "0.1"); ok("third", "0.333333333333333")
    ok("exponent_leading_zeros", "1e0000000000000000000005"); ok("tpch_price", "104949.50"); ok("19_digits_all_but_one_zero", "0.000000000000000001")
    slow("2_pow_53", str(1 << 53)); slow("2_pow_53_plus_1", str((1 << 53) + 1)); slow("17_digits", "12345678901234567"); slow("20_digits", "12345678901234567890")
    slow("21_digits_integer", "1" + "0" * 20); slow("e23", "1e23"); slow("e_minus_23", "1e-23"); slow("e308", "1e308"); slow("e_minus_308", "1e-308"); slow("e309_is_inf", "1e309")
    slow("trailing_zeros_past_19_digits", "1." + "0" * 22); slow("22_fraction_digits", "0.1234567890123456789012"); slow("1e_minus_24_written_out", "0." + "0" * 23 + "1")
    slow("exponent_2_pow_32", "1e4294967296"); slow("exponent_2_pow_32_plus_1", "1e4294967297"); slow("exponent_2_pow_31", "1e2147483648"); slow("exponent_minus_2_pow_32", "1e-4294967296")
    slow("exponent_of_20_nines", "1e99999999999999999999"); slow("exponent_2_pow_64_plus_5", "1e18446744073709551621"); slow("exponent_minus_2_pow_32_plus_22", "1e-4294967274")
    slow("19_digits_e_minus_19", "1234567890123456789e-19"); slow("fraction_moves_exponent_out_of_range", "0.1e-22"); slow("written_zeros_move_exponent_out_of_range", "100.0e-23")
    bad("lone_minus", b"-"); bad("lone_plus", b"+"); bad("lone_dot", b"."); bad("minus_dot", b"-."); bad("no_mantissa", b"e5"); bad("sign_no_mantissa", b"-e5"); bad("dot_no_mantissa", b".e5")
    bad("no_exponent_digits", b"1e"); bad("exponent_sign_only", b"1e+"); bad("exponent_minus_only", b"1e-"); bad("inf", b"inf"); bad("minus_inf", b"-inf"); bad("infinity", b"Infinity")
    bad("nan", b"nan"); bad("NaN", b"NaN"); bad("garbage_after_exponent", b"1e5x"); bad("two_dots", b"1.2.3"); bad("letter", b"1x"); bad("two_signs", b"--1"); bad("fraction_exponent", b"1e5.0")
    bad("two_exponents", b"1e5e5"); bad("leading_space", b" 1"); bad("trailing_space", b"1 "); bad("underscore", b"1_0"); bad("hex_float", b"0x1p3"); bad("slash_below_0", b"1/")
    bad("colon_above_9", b"1:"); bad("d_exponent", b"1d5"); bad("comma_decimal", b"1;5"); bad("empty_required", b"", why=REQUIRED); bad("lone_minus_nullable", b"-", nullable=True)
    out.append(Case("float64/empty_nullable", "Float64", True, b"", NULL))
    out.append(Case("float64/value_in_nullable", "Float64", True, b"-2.5e-3", -2.5e-3))
    return out


def _bool_cases():
    out = [Case("boolean/" + f.decode(), "Boolean", False, f, v) for f, v in BOOL_SPELLINGS.items()]
    # tRuE: arrow-csv's rule for mixed case could not be established from the reference's tree (its crates are not vendored); the
    # device reads the six spellings the checker reads and refuses every other one, which can never store a wrong value
    for f in (b"tXYZ", b"fabcd", b"t", b"f", b"1", b"0", b"tRuE", b"tRUE", b"FALSe", b"fALSE", b"truee", b"tru", b"falsee", b"fals", b"yes", b"true ", b" true", b"T", b"Tru3"):
        out.append(Case("boolean/refused_%s" % f.decode().replace(" ", "_space_"), "Boolean", False, f, refused(*PARSE)))
    out.append(Case("boolean/refused_empty_required", "Boolean", False, b"", refused(*REQUIRED)))
    out.append(Case("boolean/empty_nullable", "Boolean", True, b"", NULL))
    out.append(Case("boolean/true_in_nullable", "Boolean", True, b"true", True))
    out.append(Case("boolean/false_in_nullable", "Boolean", True, b"FALSE", False))
    out.append(Case("boolean/refused_tXYZ_nullable", "Boolean", True, b"tXYZ", refused(*PARSE)))
    return out


def _utf8_cases():
    out = []
    for name, f in (("empty_required", b""), ("one_byte", b"a"), ("two_byte_character", "café".encode()), ("three_and_four_byte_characters", "☃ \U0001F600".encode()),
                    ("300_bytes", bytes(range(0x30, 0x7B)) * 4), ("16_bytes", b"0123456789abcdef"), ("spaces", b"  "), ("looks_like_a_number", b"-12.5e3"),
                    ("the_word_null", b"NULL"), ("tab", b"a\tb"), ("pipe", b"a|b")):
        out.append(Case("utf8/" + name, "Utf8", False, f, f.decode()))
    out.append(Case("utf8/empty_nullable", "Utf8", True, b"", NULL))
    out.append(Case("utf8/value_in_nullable", "Utf8", True, b"x" * 17, "x" * 17))
    out.append(Case("utf8/refused_quote", "Utf8", False, b'a"b', refused(*QUOTED, value='a"b')))
    out.append(Case("utf8/refused_quoted_field", "Utf8", False, b'"ab"', refused(*QUOTED, value='"ab"')))
    # csv-core (behind arrow-csv) and Arrow C++ both end a record at a lone carriage return; the device splits lines at line feeds
    # only, so it refuses the byte instead of keeping it inside a value that neither reader returns
    out.append(Case("utf8/refused_lone_carriage_return", "Utf8", False, b"a\rb", refused(*BARE_CR)))
    out.append(Case("utf8/refused_carriage_return_before_the_delimiter", "Utf8", False, b"ab\r", refused(*BARE_CR)))
    return out


@functools.lru_cache(maxsize=None)
def corpus():
    return tuple(_int_cases() + _date_cases() + _dec_cases() + _float_cases() + _bool_cases() + _utf8_cases())


def is_refused(c):
    return isinstance(c.expect, Refused)


def cases(prefix="", refused_only=None):
    return [c for c in corpus() if c.name.startswith(prefix) and (refused_only is None or is_refused(c) == refused_only)]


ROW = ("row", "Int32", False)


def field_schema(c):
    return [("v", c.ctype, c.nullable), ROW]


@functools.lru_cache(maxsize=None)
def batches():
    """[(label, schema, [cases], text)]: the valid cases of one column type and nullability as one file, a case per line, its number
    in a second column"""
    groups = {}
    for c in cases(refused_only=False):
        groups.setdefault((type_key(c.ctype), c.nullable), []).append(c)
    out = []
    for (key, nullable), cs in groups.items():
        text = b"".join(c.field + b",%d\n" % i for i, c in enumerate(cs))
        out.append(("%s%s" % (key, "_nullable" if nullable else ""), field_schema(cs[0]), cs, text))
    return tuple(out)


def file_of(c, row=7):
    """a refused (or any) case as a file of its own: a clean line before and after the case's"""
    clean = {"Int32": b"1", "Int64": b"1", "Date32": b"2001-02-03", "Float64": b"1.5", "Boolean": b"true", "Utf8": b"ok"}.get(type_key(c.ctype), b"0")
    return clean + b",6\n" + c.field + b",%d\n" % row + clean + b",8\n"


def column_values(col, ctype):
    """a pyarrow column as the corpus records values: ints, unscaled ints, days, bools, text, floats; None where it is NULL"""
    import pyarrow as pa
    col = col.combine_chunks() if hasattr(col, "combine_chunks") else col
    if ctype == "Date32":
        return col.cast(pa.int32()).to_pylist()
    if isinstance(ctype, dict):
        return [None if v is None else unscaled(v, ctype["Decimal128"][1]) for v in col.to_pylist()]
    return col.to_pylist()


def same_value(got, want):
    """exact; a float by its bits (-0.0 is not 0.0)"""
    if want is NULL or got is None:
        return want is NULL and got is None
    if isinstance(want, float):
        return isinstance(got, float) and float_bits(got) == float_bits(want)
    return type(got) is type(want) and got == want


# ---------------------------------------------------------------- layout cases: whole files, the smallest that reach a boundary
BNI = [("b", "Boolean", False), ("n", "Int64", True), ("i", "Int32", False)]
KS = [("k", "Int64", False), ("s", "Utf8", False)]
KSD = [("k", "Int64", False), ("s", "Utf8", False), ("d", dec(15, 2), False)]
CHUNK = 1 << 16          # bytes per block of the line splitter (gpuq_csv_decode)
LDS_BYTES = 40 * 1024    # CSV_LDS_BYTES: the byte range of a block's 256 lines is staged when it fits


def _bni_lines(n):
    return [b"%s,%s,%d" % ((b"true", b"FALSE", b"True", b"false", b"TRUE")[(j * 7) % 5] if (j * 11) % 3 else b"False", b"" if j % 5 == 0 or j in (63, 64, 255, 256) else b"%d" % (j * j - 1000), j)
            for j in range(n)]


def _ks_text_with_line_end_at(at, straddle=False):
    """KS lines up to a line whose '\\n' is byte `at` of the text (or, straddling, a line that starts before `at` and ends 20 bytes
    after it), then five more"""
    text, j = bytearray(), 0
    while len(text) + 120 < at:
        text += b"%d,%s\n" % (j * 1000003, b"abcdefghijklmnopqrstuvwxyz"[:1 + j % 26] * (1 + j % 2))
        j += 1
    head = b"%d," % j
    text += head + b"y" * ((at + 20 if straddle else at) - len(text) - len(head)) + b"\n"
    for k in range(5):
        text += b"%d,tail%d\n" % (-k, k)
    return bytes(text)


def _ksd_block(first, line_bytes, n=256):
    """n KSD lines of exactly line_bytes bytes each (the '\\n' included)"""
    out = bytearray()
    for j in range(first, first + n):
        head, tail = b"%d," % (j * 7919), b",%d.%02d\n" % (j * 31, j % 100)
        out += head + bytes([0x61 + (j + k) % 26 for k in range(line_bytes - len(head) - len(tail))]) + tail
    assert len(out) == n * line_bytes
    return bytes(out)


@functools.lru_cache(maxsize=None)
def layouts():
    out = []

    def add(name, schema, text, expect="rows", delimiter=b",", header=False, projection=None, pyarrow=True):
        out.append(Layout(name, schema, text, delimiter, header, projection, expect, pyarrow))
    for n in (63, 64, 65, 255, 256, 257):      # the 64-row ballot words of validity and Boolean columns, the 256-line block
        add("rows/%d" % n, BNI, b"\n".join(_bni_lines(n)) + b"\n")
    add("rows/257_crlf_unterminated", BNI, b"\r\n".join(_bni_lines(257)))
    add("chunk/line_end_is_the_last_byte_of_a_chunk", KS, _ks_text_with_line_end_at(CHUNK - 1))
    add("chunk/line_end_is_the_first_byte_of_a_chunk", KS, _ks_text_with_line_end_at(CHUNK))
    add("chunk/line_straddles_the_chunks", KS, _ks_text_with_line_end_at(CHUNK, straddle=True))
    add("chunk/crlf_split_by_the_chunks", KS, _crlf_split_text())
    i32 = [("v", "Int32", False)]
    short = [b"%d" % ((j * 37) % (10, 100, 1000)[j % 3]) for j in range(1000)]      # 1 to 3 bytes a line: a lane's 16 bytes hold several line ends
    add("short/lines_of_1_to_3_bytes", i32, b"\n".join(short) + b"\n")
    add("short/lines_of_1_byte", i32, b"".join(b"%d\n" % (j % 10) for j in range(700)))
    add("short/lines_of_1_to_3_bytes_crlf", i32, b"\r\n".join(short[:300]) + b"\r\n")
    # 256 lines just under 40 KiB are staged into LDS, the next 256 just over it are read in place, in one file (and the other way round)
    under, over = _ksd_block(0, 159), _ksd_block(256, 161)
    add("lds/staged_then_in_place", KSD, under + over + _ksd_block(512, 40, n=70))
    add("lds/in_place_then_staged", KSD, over + _ksd_block(256 + 256, 159) + _ksd_block(900, 40, n=3))
    add("lds/exactly_the_budget", KSD, _ksd_block(0, 160) + _ksd_block(256, 160, n=100))
    add("ends/crlf", KS, b"1,a\r\n2,bc\r\n3,\r\n")
    add("ends/unterminated_last_line", KS, b"1,a\n2,bc")
    add("ends/unterminated_last_line_with_carriage_return", KS, b"1,a\r\n2,bc\r")
    add("ends/one_line_crlf", KS, b"1,x\r\n")
    add("ends/header_with_no_rows", KS, b"k,s\n", header=True)
    add("ends/unterminated_header_with_no_rows", KS, b"k,s", header=True, pyarrow=False)      # (pyarrow calls it an empty file)
    add("ends/header_crlf_then_rows", KS, b"k,s\r\n5,five\r\n", header=True)
    add("ends/empty_file", KS, b"")
    tbl = [("a", "Int64", False), ("b", "Utf8", False), ("c", dec(15, 2), True)]
    add("fields/trailing_delimiter", tbl, b"1|x|2.50|\n2||\n3|z|-1|\n", delimiter=b"|", pyarrow=False)
    add("fields/trailing_delimiter_on_some_lines", tbl, b"1|x|2.50|\n2|y|\n3|z|-1\n", delimiter=b"|", pyarrow=False)
    add("fields/refused_two_trailing_delimiters", tbl, b"1|x|2.50||\n", refused(*COUNT), delimiter=b"|", pyarrow=False)
    add("fields/refused_one_field_short", tbl, b"1|x|2.50\n2|y\n", refused(*COUNT), delimiter=b"|")
    add("fields/refused_one_field_more", tbl, b"1|x|2.50\n2|y|1|1\n", refused(*COUNT), delimiter=b"|")
    # a projection reads only its own fields: what stands in the others is not looked at -- but for the line's structure: the
    # field count holds for every line, and a quote anywhere in a line is refused (a quoted field could hold a delimiter)
    wide = [("a", "Int64", False), ("b", "Int64", False), ("c", "Float64", False), ("d", "Date32", False), ("e", "Utf8", False), ("f", dec(5, 2), False), ("g", "Boolean", False)]
    junk = b"1,12x,--,2023-13-45,one,1e2,tXYZ\n-2,,1e,abcd-ef-gh,two,9999999,\n3,99999999999999999999,nan,,three,.,maybe\n"
    add("projection/skips_malformed_fields", wide, junk, projection=["a", "e"])
    add("projection/skips_malformed_fields_reordered", wide, junk, projection=["e", "a"])
    for name in ("b", "c", "d", "f", "g"):
        add("projection/refused_when_the_malformed_field_is_projected_" + name, wide, junk, refused(*PARSE), projection=["a", name])
    add("projection/refused_field_count_of_a_line_it_skips_most_of", wide, b"1,2,3.0,2023-01-01,one,1.00,true\n2,2,3.0,2023-01-01,two,1.00\n", refused(*COUNT), projection=["a"])
    add("projection/refused_quote_in_a_skipped_field", wide, b'1,2,3.0,2023-01-01,"one",1.00,true\n', refused(*QUOTED), projection=["a"], pyarrow=False)
    # blank lines: Arrow C++ skips them (and so does the csv crate behind arrow-csv); the device never makes a row of one: it refuses the file
    n1, u1 = [("v", "Int64", True)], [("v", "Utf8", False)]
    for tag, schema, a, b in (("one_nullable_column", n1, b"1", b"2"), ("one_required_utf8_column", u1, b"a", b"b"), ("three_columns", BNI, b"true,1,1", b"false,,2")):
        add("blank/refused_in_the_middle_" + tag, schema, a + b"\n\n" + b + b"\n", refused(*BLANK))
        add("blank/refused_at_the_end_" + tag, schema, a + b"\n" + b + b"\n\n", refused(*BLANK))
        add("blank/refused_crlf_in_the_middle_" + tag, schema, a + b"\r\n\r\n" + b + b"\r\n", refused(*BLANK))
    add("blank/refused_first_line_one_nullable_column", n1, b"\n1\n", refused(*BLANK))
    add("blank/refused_only_line_one_nullable_column", n1, b"\n", refused(*BLANK))
    add("blank/refused_after_the_header", KS, b"k,s\n\n1,a\n", refused(*BLANK), header=True)
    add("cr/refused_lone_carriage_return_in_a_line", KS, b"1,a\rb\n2,c\n", refused(*BARE_CR))
    add("cr/refused_carriage_return_line_ends_only", KS, b"1,a\r2,b\r", refused(*BARE_CR))
    add("cr/refused_two_carriage_returns_before_the_line_feed", KS, b"1,a\r\r\n2,b\r\n", refused(*BARE_CR))
    return tuple(out)


def _crlf_split_text():
    """CRLF lines, the '\\r' of one the last byte of the first chunk and its '\\n' the first byte of the second"""
    text, j = bytearray(), 0
    while len(text) + 120 < CHUNK:
        text += b"%d,%s\r\n" % (j, b"q" * (3 + j % 40))
        j += 1
    head = b"%d," % j
    text += head + b"z" * (CHUNK - 1 - len(text) - len(head)) + b"\r\n"
    text += b"77,after\r\n78,last"
    return bytes(text)


def layout(name):
    return [x for x in layouts() if x.name == name][0]
