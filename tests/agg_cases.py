"""Workloads, apps and model specs shared by tests/test_aggregators.py (CPU) and
tests/test_gpu_aggregators.py: one generated stream, an app text and the
matching tests/agg_model.py Spec built side by side from one description, the
runners, and the known answers under tests/golden/kat_aggregators/ with their
hand-written Specs (the model does not read query text).
"""
import json
import os
import re

import numpy as np

import agg_model as am
import minmax_cases as mc
from siddhi_amd import runtime as rt

ROOT = mc.ROOT
KAT_DIR = os.path.join(ROOT, "tests", "golden", "kat_aggregators")

NAMES = ["i", "k", "g", "x", "y", "f", "d", "et", "b", "s"]
ATTR = {n: j for j, n in enumerate(NAMES)}
TYPE = {"i": am.T_LONG, "k": am.T_STRING, "g": am.T_STRING, "x": am.T_INT, "y": am.T_LONG, "f": am.T_FLOAT,
        "d": am.T_DOUBLE, "et": am.T_LONG, "b": am.T_BOOL, "s": am.T_STRING}
S = ("@app:playback define stream S (i long, k string, g string, x int, y long, f float, d double, et long, "
     "b bool, s string); ")
NULLABLE = ["x", "y", "f", "d", "b", "s"]       # rows of the stream's null table
T0 = mc.T0
PUSHES = [(0, 300, 1), (300, 1040, 37), (1040, 3088, 1024)]   # (first event, end, call size)
N = PUSHES[-1][1]


def make_stream(n=N, seed=0, domain=8, nkeys=1, ngroups=1, nulls=False, special=False):
    """Values are drawn from 0..domain-1 and mapped to non-dyadic floats and
    doubles (v / 3, v / 7 + 0.1: sums and means round at every step), so keys
    repeat and a sliding window often holds equal values -- the residue of
    stdDeviation is then all there is, of either sign.  nulls: a fifth of
    x / y / f / d / b / s are null.  special: f and d also take NaN, 0.0 and
    -0.0.  With hundreds of groups under one short sliding window every group's
    state drains to count 0 and refills, over and over."""
    rng = np.random.default_rng(seed)
    v = rng.integers(0, domain, n)
    d = {"i": np.arange(n, dtype=np.int64), "k": rng.integers(0, nkeys, n), "g": rng.integers(0, ngroups, n),
         "x": v.astype(np.int32), "y": v.astype(np.int64) * 3_000_000_007 - 5, "f": (v / 3.0).astype(np.float32),
         "d": v / 7.0 + 0.1, "b": rng.integers(0, 4, n) != 0, "s": rng.integers(0, domain, n)}
    if special:
        pick = rng.integers(0, 12, n)
        for c, nan, z in (("d", np.nan, np.float64(0.0)), ("f", np.float32(np.nan), np.float32(0.0))):
            d[c] = np.where(pick == 0, nan, np.where(pick == 1, -z, np.where(pick == 2, z, d[c])))
    step = rng.choice([0, 0, 1, 1, 2, 3, 50, -1], n)
    et = np.maximum.accumulate(np.cumsum(np.where(step < 0, 0, step))) + 5000
    d["et"] = (et + np.where(step < 0, -1, 0)).astype(np.int64)
    d["null"] = (rng.integers(0, 5, (len(NULLABLE), n)) == 0) if nulls else np.zeros((len(NULLABLE), n), bool)
    return d


def as_events(d):
    nul = d["null"]
    out = []
    for j in range(len(d["i"])):
        def val(c, conv):
            return None if nul[NULLABLE.index(c)][j] else conv(d[c][j])
        out.append((T0 + j, [int(d["i"][j]), "K%04d" % d["k"][j], "G%04d" % d["g"][j], val("x", int), val("y", int),
                             val("f", np.float32), val("d", float), int(d["et"][j]), val("b", bool),
                             val("s", lambda q: "P%05d" % q)]))
    return out


def as_batch(d, a, b, call, dictionary):
    def ids(fmt, col):
        return np.array([dictionary.id(fmt % q) for q in d[col][a:b]], np.uint32)
    offs = np.append(np.arange(0, b - a, call, dtype=np.int64), np.int64(b - a))
    ts = T0 + np.arange(a, b, dtype=np.int64)
    cols = {"i": d["i"][a:b].copy(), "k": ids("K%04d", "k"), "g": ids("G%04d", "g"), "x": d["x"][a:b].copy(),
            "y": d["y"][a:b].copy(), "f": d["f"][a:b].astype(np.float32), "d": d["d"][a:b].astype(np.float64),
            "et": d["et"][a:b].copy(), "b": d["b"][a:b].astype(np.uint8), "s": ids("P%05d", "s")}
    nul = []
    for n in NAMES:
        m = d["null"][NULLABLE.index(n)][a:b] if n in NULLABLE else None
        nul.append(m.astype(np.uint8) if m is not None and m.any() else None)
    return rt.ColumnBatch(ts, [cols[n] for n in NAMES], nul, offs)


# ---------------------------------------------------------------- app + spec
_AGG = re.compile(r"^(\w+)\((\w*)\)$")
WINDOWS = {None: None, "length(4)": ("length", 4), "length(64)": ("length", 64), "length(5000)": ("length", 5000),
           "lengthBatch(3)": ("lengthBatch", 3), "externalTime(et, 20)": ("externalTime", ATTR["et"], 20)}


class Case:
    """As minmax_cases.Case, over this module's stream and agg_model's Spec."""

    def __init__(self, name, window, select, events="current", group=False, part=False, having=None, stream=None,
                 pushes=PUSHES):
        self.name, self.stream, self.pushes = name, stream or {}, pushes
        # no aggregator the oracle knows returns a BOOL to compare in `having`
        self.oracle_ok = not (having is not None and isinstance(having[2], bool))
        aggs, outs, texts = [], [], []

        def agg(text):
            kind, arg = _AGG.match(text).groups()
            aggs.append((kind, ATTR[arg] if arg else None, TYPE[arg] if arg else am.T_LONG))
            return len(aggs) - 1

        for n, item in enumerate(select):
            if isinstance(item, tuple):
                text, parts, fn = item
                idx = [agg(p) for p in parts]
                outs.append(("fn", lambda d, a, idx=idx, fn=fn: fn(*[a[q] for q in idx])))
            elif _AGG.match(item):
                text = item
                outs.append(("agg", agg(item)))
            else:
                text = item
                outs.append(("attr", ATTR[item]))
            texts.append("%s as c%d" % (text, n))
        hav_text, hav = "", None
        if having is not None:
            col, op, const = having
            o = outs[col]
            assert o[0] == "agg"
            hav_text = "having c%d %s %s " % (col, op, str(const).lower())
            cmp = {">": lambda a, b: a > b, "<": lambda a, b: a < b, "==": lambda a, b: a == b}[op]
            # a null operand compares false (C/executor/condition/compare)
            hav = lambda d, a, q=o[1]: a[q] is not None and bool(cmp(a[q], const))
        q = "@info(name = 'q') from S%s select %s %s%sinsert %sinto O;" % (
            "#window.%s" % window if window else "", ", ".join(texts), "group by g " if group else "", hav_text,
            mc.EVENTS[events])
        self.app = S + ("partition with (k of S) begin %s end;" % q if part else q)
        self.spec = am.Spec(WINDOWS[window], aggs, outs, events, ATTR["g"] if group else None,
                            ATTR["k"] if part else None, hav, None)

    def with_aggs(self, swap):
        """The same query with aggregators the oracle knows; (kind, attr) pairs
        the oracle's kinds cannot take (sum of a bool or a string) move to d."""
        c = Case.__new__(Case)
        c.name, c.stream, c.pushes, c.oracle_ok = self.name, self.stream, self.pushes, self.oracle_ok
        c.app = self.app
        for a, b in swap.items():
            c.app = re.sub(r"\b%s\((b|s)\)" % a, b + "(d)", c.app)
            c.app = re.sub(r"\b%s\(" % a, b + "(", c.app)
        s = self.spec
        aggs = [(swap.get(k, k), ATTR["d"] if k in swap and a in (ATTR["b"], ATTR["s"]) else a,
                 am.T_DOUBLE if k in swap and a in (ATTR["b"], ATTR["s"]) else t) for k, a, t in s.aggs]
        c.spec = am.Spec(s.window, aggs, s.outputs, s.events, s.group, s.partition, s.having, s.where)
        return c


def band(a, s):
    return None if a is None or s is None else a + 2.0 * s


def twice(n):
    return None if n is None else n * 2


SHAPES = [
    Case("none-stddev-types", None, ["i", "stdDev(x)", "stdDev(y)", "stdDev(f)", "stdDev(d)"], stream={"nulls": True}),
    Case("length4-stddev-all", "length(4)", ["i", "stdDev(d)", "stdDev(f)", "stdDev(x)", "stdDev(y)"], "all",
         stream={"nulls": True}),
    Case("length4-stddev-expired", "length(4)", ["i", "stdDev(d)", "count()"], "expired"),
    Case("length4-stddev-special", "length(4)", ["i", "stdDev(d)", "stdDev(f)"], "all", stream={"special": True}),
    Case("length4-group700", "length(4)", ["g", "stdDev(d)", "distinctCount(x)", "and(b)"], "all", group=True,
         stream={"ngroups": 700, "nulls": True}),
    Case("length64-group40", "length(64)", ["g", "i", "stdDev(d)", "distinctCount(s)", "or(b)"], "all",
         group=True, stream={"ngroups": 40}),
    Case("lengthBatch3-all", "lengthBatch(3)", ["i", "stdDev(d)", "distinctCount(x)", "and(b)", "or(b)"], "all",
         stream={"nulls": True}),
    Case("lengthBatch3-group-current", "lengthBatch(3)", ["g", "stdDev(f)", "distinctCount(d)", "or(b)"], group=True,
         stream={"ngroups": 3}),
    Case("lengthBatch3-group-expired", "lengthBatch(3)", ["g", "stdDev(x)", "distinctCount(s)", "and(b)"], "expired",
         group=True, stream={"ngroups": 3, "nulls": True}),
    Case("externalTime-all", "externalTime(et, 20)", ["i", "et", "stdDev(d)", "distinctCount(y)", "and(b)"], "all",
         stream={"nulls": True}),
    Case("externalTime-group-current", "externalTime(et, 20)", ["g", "stdDev(y)", "distinctCount(f)"], group=True,
         stream={"ngroups": 700}),
    Case("none-group", None, ["g", "stdDev(d)", "distinctCount(x)", "and(b)", "or(b)"], group=True,
         stream={"ngroups": 700, "nulls": True}),
    Case("distinct-types", "length(64)", ["i", "distinctCount(x)", "distinctCount(y)", "distinctCount(f)",
                                          "distinctCount(d)", "distinctCount(s)", "distinctCount(b)"], "all",
         stream={"nulls": True, "special": True, "domain": 40}),
    Case("distinct-expired-special", "length(4)", ["i", "distinctCount(d)", "distinctCount(f)"], "expired",
         stream={"special": True, "nulls": True}),
    Case("bool-nulls", "length(4)", ["i", "and(b)", "or(b)"], "all", stream={"nulls": True}),
    Case("partition-length4", "length(4)", ["k", "i", "stdDev(d)", "distinctCount(x)", "or(b)"], "all", part=True,
         stream={"nkeys": 5, "nulls": True}),
    Case("partition-group-none", None, ["k", "g", "stdDev(f)", "distinctCount(s)", "and(b)"], group=True, part=True,
         stream={"nkeys": 5, "ngroups": 40}),
    Case("mixed-five", "length(4)", ["i", "stdDev(d)", "distinctCount(x)", "max(x)", "sum(x)", "count()"], "all",
         stream={"nulls": True}),
    Case("having-stddev", "length(4)", ["i", "stdDev(d)", "distinctCount(x)"], "all", having=(1, ">", 0.25)),
    Case("having-distinct", "length(64)", ["i", "distinctCount(s)", "and(b)"], "all", having=(1, ">", 7)),
    Case("having-or", "length(4)", ["i", "or(b)", "stdDev(x)"], "all", having=(1, "==", True), stream={"nulls": True}),
    Case("expression", "length(64)", ["i", ("avg(d) + 2.0 * stdDev(d)", ["avg(d)", "stdDev(d)"], band),
                                      ("distinctCount(x) * 2", ["distinctCount(x)"], twice)], "all"),
]
# the oracle knows sum / avg / count: the model's windows, partitions and selector are pinned with them
TO_ORACLE = {"stdDev": "avg", "distinctCount": "count", "and": "count", "or": "sum", "max": "sum"}


def shape(name):
    return next(c for c in SHAPES if c.name == name)


# ---------------------------------------------------------------- runners
def model_chunks(spec, d, pushes=PUSHES):
    m = am.Model(spec)
    evs = as_events(d)
    out = []
    for a, b, call in pushes:
        out.extend(m.run([evs[x:min(x + call, b)] for x in range(a, b, call)]))
    return am.norm_chunks(out)


def runtime_chunks(app, d, engine_factory=None, pushes=PUSHES, snapshot_after=None):
    """minmax_cases.runtime_chunks over this module's batches."""
    got = []
    r = mc.new_runtime(app, got, engine_factory)
    for p, (a, b, call) in enumerate(pushes):
        r.getInputHandler("S").send_batch(as_batch(d, a, b, call, r.dictionary))
        if snapshot_after == p:
            image = r.snapshot()
            r.shutdown()
            r = mc.new_runtime(app, got, engine_factory)
            r.restore(image)
    r.shutdown()
    return got


assert_same = mc.assert_same


# ---------------------------------------------------------------- time window on a stepped wall clock
def time_case(agg_texts, n=160, seed=4):
    """A wall-clock app in tests/kat_runner.py's form: time(1 sec), one event
    per send, pauses of 10 .. 400 ms between sends and a last one that drains
    the window.  Every time is a multiple of the runner's 10 ms tick, so each
    expiry fires at its own due time, as the model's timers do.  Returns
    (case, Spec)."""
    rng = np.random.default_rng(seed)
    app = ("define stream S (x int, d double, b bool); @info(name = 'query1') from S#window.time(1 sec) select %s "
           "insert all events into O;" % ", ".join("%s as c%d" % (t, n) for n, t in enumerate(agg_texts)))
    cols = {"x": (0, am.T_INT), "d": (1, am.T_DOUBLE), "b": (2, am.T_BOOL)}
    aggs = []
    for t in agg_texts:
        kind, arg = _AGG.match(t).groups()
        aggs.append((kind, cols[arg][0], cols[arg][1]) if arg else (kind, None, am.T_LONG))
    clock, sends = 1_000_000, []
    for j in range(n):
        clock += int(rng.choice([10, 10, 20, 50, 130, 400]))
        sends.append({"time": clock})
        v = int(rng.integers(0, 6))
        sends.append({"stream": "S", "ts": clock,
                      "data": [None if rng.integers(0, 6) == 0 else {"int": v}, v / 7.0 + 0.1, bool(rng.integers(0, 3))]})
    sends.append({"time": clock + 1500})
    case = {"name": "time-window", "app": app, "callback": {"kind": "query", "name": "query1"}, "sends": sends}
    return case, am.Spec(("time", 1000), aggs, [("agg", j) for j in range(len(aggs))], "all")


def collector_chunks(col):
    """A kat_runner Collector's (or model_collector's) callbacks, values in norm form."""
    return [([[am.norm(v) for v in e.getData()] for e in cur], [[am.norm(v) for v in e.getData()] for e in rem])
            for cur, rem in col.chunks]


# ---------------------------------------------------------------- known answers
def load_kats():
    cases = []
    for f in sorted(os.listdir(KAT_DIR)):
        if f.endswith(".json"):
            with open(os.path.join(KAT_DIR, f)) as fp:
                cases.extend(json.load(fp))
    return cases


def short(case):
    return case["name"].split(".")[-1]


KATS = load_kats()
RUN_KATS = [c for c in KATS if "expected_exception" not in c]
FAIL_KATS = [c for c in KATS if "expected_exception" in c]


def _kat_specs():
    sd = "StdDevAttributeAggregatorExecutorTestCase.stdDevAggregatorTest%d"
    out = {sd % 1: am.Spec(None, [("stdDev", 1, am.T_DOUBLE)], [("agg", 0)], group=0)}
    for n, w in ((2, 1), (3, 3), (4, 6), (5, 6)):
        out[sd % n] = am.Spec(("lengthBatch", w), [("stdDev", 1, am.T_DOUBLE)], [("agg", 0)], group=0)
    out[sd % 6] = am.Spec(("length", 3), [("stdDev", 1, am.T_DOUBLE)], [("agg", 0)], "all", group=0)
    out["DistinctCountAttributeAggregatorExecutorTestCase.distinctCountTest"] = am.Spec(
        ("time", 5000), [("distinctCount", 2, am.T_STRING)], [("attr", 1), ("attr", 2), ("agg", 0)], group=1,
        having=lambda d, a: a[0] > 3)
    for cap, fn, names in (("And", "and", ["TrueOnly", "FalseOnly", "TrueFalse", "MoreEventsBatch"]),
                           ("Or", "or", ["TrueOnly", "FalseOnly", "TrueFalse", "MoreEventsBatch"])):
        for nm, w in zip(names, (3, 4, 4, 2)):
            test = "test%sAggregator%sScenario" % ("OR" if cap == "Or" and nm == "MoreEventsBatch" else cap, nm)
            out["%sAggregatorExtensionTestCase.%s" % (cap, test)] = am.Spec(
                ("lengthBatch", w), [(fn, 1, am.T_BOOL)], [("attr", 0), ("agg", 0)], "all", group=0)
    plain = lambda fn: am.Spec(None, [(fn, 1, am.T_BOOL)], [("agg", 0)])
    out["AndAggregatorExtensionTestCase.andAggregatorTest6"] = plain("and")
    out["OrAggregatorExtensionTestCase.orAggregatorTest2"] = plain("or")
    out["OrAggregatorExtensionTestCase.orAggregatorTest3"] = plain("or")
    return out


KAT_SPECS = _kat_specs()


class _Ev:
    def __init__(self, data):
        self.data = data

    def getData(self):  # noqa: N802
        return self.data


class _Col:
    def __init__(self):
        self.in_events, self.remove_events, self.chunks = [], [], []


def model_collector(case, spec=None):
    """The case's sends through the model, collected as tests/kat_runner.py's callbacks collect."""
    m = am.Model(spec or KAT_SPECS[case["name"]])
    col = _Col()
    stream_cb = case["callback"]["kind"] == "stream"

    def take(chunks):
        for c in chunks:
            cur = [_Ev([float(v) if isinstance(v, np.floating) else v for v in vals])
                   for t, ts, vals in c if t == am.CURRENT or stream_cb]
            rem = [_Ev(list(vals)) for t, ts, vals in c if t == am.EXPIRED and not stream_cb]
            col.chunks.append((cur, rem))
            col.in_events.extend(cur)
            col.remove_events.extend(rem)

    for s in case["sends"]:
        if "time" in s:
            take(m.advance(s["time"]))
            continue
        data = []
        for v in s["data"]:
            if isinstance(v, dict):
                (k, x), = v.items()
                v = np.float32(x) if k == "float" else x
            data.append(v)
        take(m.advance(s["ts"]))
        take(m.run([[(s["ts"], data)]]))
    return col


def check_kat(case, col):
    """tests/kat_runner.check_case for these files: the count, and every
    expected row -- doubles within the case's `epsilon`, the absolute bound the
    reference's own test asserts with (Math.abs(expected - actual) < epsilon),
    everything else exactly."""
    errs = []
    if len(col.in_events) != case["expected_count"]:
        errs.append("count %d != expected %d" % (len(col.in_events), case["expected_count"]))
    eps = case.get("epsilon")
    for exp in case["expected_rows"]:
        if exp["n"] - 1 >= len(col.in_events):
            errs.append("missing event #%d" % exp["n"])
            continue
        d = col.in_events[exp["n"] - 1].getData()
        ok = len(d) == len(exp["data"])
        for e, a in zip(exp["data"], d):
            if isinstance(e, dict):               # {"long": 4}: a typed integer
                (_, e), = e.items()
            if isinstance(e, float) and eps is not None:
                ok = ok and isinstance(a, float) and abs(e - a) < eps
            else:
                ok = ok and type(e) is type(a) and e == a
        if not ok:
            errs.append("event %d: %r != expected %r" % (exp["n"], d, exp["data"]))
    return errs
