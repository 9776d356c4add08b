"""Workloads, apps and model specs shared by tests/test_minmax.py (CPU) and
tests/test_gpu_minmax.py: one generated stream, an app text and the matching
tests/minmax_model.py Spec built side by side from the same description, and
the runner that takes a SiddhiManager's callbacks in the model's form.

The known answers under tests/golden/kat_minmax/ are loaded here too, each
with its hand-written Spec (the model does not read query text).
"""
import json
import os
import re

import numpy as np

import minmax_model as mm
from siddhi_amd import runtime as rt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KAT_DIR = os.path.join(ROOT, "tests", "golden", "kat_minmax")

ATTR = {"i": 0, "k": 1, "g": 2, "x": 3, "y": 4, "f": 5, "d": 6, "et": 7}
TYPE = {"i": mm.T_LONG, "k": mm.T_STRING, "g": mm.T_STRING, "x": mm.T_INT, "y": mm.T_LONG, "f": mm.T_FLOAT,
        "d": mm.T_DOUBLE, "et": mm.T_LONG}
S = "@app:playback define stream S (i long, k string, g string, x int, y long, f float, d double, et long); "
T0 = 1_000_000                                  # playback timestamps: T0 + event index
PUSHES = [(0, 1000, 1), (1000, 2000, 37), (2000, 3000, 1024)]   # (first event, end, call size)
# the quirk is visible in the EXPIRED rows of one-event calls (a larger call's chunk shows its last row only)
QUIRK_PUSHES = [(0, 2400, 1), (2400, 2700, 37), (2700, 3000, 1024)]


def make_stream(n=3000, seed=0, domain=8, nkeys=1, ngroups=1, nulls=False, special=False):
    """domain: values are drawn from 0..domain-1 (duplicates: the deque's
    removeFirstOccurrence quirk fires), 0 = pairwise distinct values.
    nulls: a fifth of x / y / f / d are null.  special: d also takes NaN and -0.0."""
    rng = np.random.default_rng(seed)
    v = rng.integers(0, domain, n) if domain else rng.permutation(n) - n // 3
    d = {"i": np.arange(n, dtype=np.int64), "k": rng.integers(0, nkeys, n), "g": rng.integers(0, ngroups, n),
         "x": v.astype(np.int32), "y": v.astype(np.int64) * 3_000_000_000, "f": (v / 2.0).astype(np.float32),
         "d": v / 4.0 - 0.5}
    if special:
        pick = rng.integers(0, 12, n)
        d["d"] = np.where(pick == 0, np.nan, np.where(pick == 1, -0.0, np.where(pick == 2, 0.0, d["d"])))
    step = rng.choice([0, 0, 1, 1, 2, 3, 50, -1], n)
    et = np.maximum.accumulate(np.cumsum(np.where(step < 0, 0, step))) + 5000
    d["et"] = (et + np.where(step < 0, -1, 0)).astype(np.int64)
    d["null"] = (rng.integers(0, 5, (4, n)) == 0) if nulls else np.zeros((4, n), bool)
    return d


def as_events(d):
    n = len(d["i"])
    nul = d["null"]
    out = []
    for j in range(n):
        out.append((T0 + j, [int(d["i"][j]), "K%04d" % d["k"][j], "G%04d" % d["g"][j],
                             None if nul[0][j] else int(d["x"][j]), None if nul[1][j] else int(d["y"][j]),
                             None if nul[2][j] else np.float32(d["f"][j]), None if nul[3][j] else float(d["d"][j]),
                             int(d["et"][j])]))
    return out


def as_batch(d, a, b, call, dictionary):
    kid = np.array([dictionary.id("K%04d" % x) for x in d["k"][a:b]], np.uint32)
    gid = np.array([dictionary.id("G%04d" % x) for x in d["g"][a:b]], np.uint32)
    offs = np.append(np.arange(0, b - a, call, dtype=np.int64), np.int64(b - a))
    ts = T0 + np.arange(a, b, dtype=np.int64)
    nul = [None, None, None] + [d["null"][c][a:b].astype(np.uint8) if d["null"][c][a:b].any() else None
                                for c in range(4)] + [None]
    cols = [d["i"][a:b].copy(), kid, gid, d["x"][a:b].copy(), d["y"][a:b].copy(), d["f"][a:b].copy(),
            d["d"][a:b].copy(), d["et"][a:b].copy()]
    return rt.ColumnBatch(ts, cols, nul, offs)


# ---------------------------------------------------------------- app + spec
_AGG = re.compile(r"^(\w+)\((\w*)\)$")
WINDOWS = {None: None, "length(5)": ("length", 5), "length(64)": ("length", 64), "length(3000)": ("length", 3000),
           "lengthBatch(4)": ("lengthBatch", 4), "externalTime(et, 20)": ("externalTime", ATTR["et"], 20)}
EVENTS = {"current": "", "all": "all events ", "expired": "expired events "}


class Case:
    """select: attribute names, single aggregators ("max(x)", "count()") or
    (text, [aggregators], fn(values of those aggregators)) for an expression;
    having: (output index, fn(value)) on an aggregator output of the select list."""

    def __init__(self, name, window, select, events="current", group=False, part=False, having=None, where=None,
                 stream=None, pushes=PUSHES):
        self.name, self.stream, self.pushes = name, stream or {}, pushes
        aggs, outs, texts = [], [], []

        def agg(text):
            kind, arg = _AGG.match(text).groups()
            aggs.append((kind, ATTR[arg] if arg else None, TYPE[arg] if arg else mm.T_LONG))
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
            hav_text = "having c%d %s %s " % (col, op, const)
            cmp = {">": lambda a, b: a > b, "<": lambda a, b: a < b}[op]
            # a null operand compares false (C/executor/condition/compare)
            hav = lambda d, a, q=o[1]: a[q] is not None and bool(cmp(a[q], const))
        q = "@info(name = 'q') from S%s%s select %s %s%sinsert %sinto O;" % (
            "[%s]" % where[0] if where else "", "#window.%s" % window if window else "", ", ".join(texts),
            "group by g " if group else "", hav_text, EVENTS[events])
        self.app = S + ("partition with (k of S) begin %s end;" % q if part else q)
        self.spec = mm.Spec(WINDOWS[window], aggs, outs, events, ATTR["g"] if group else None,
                            ATTR["k"] if part else None, hav, where[1] if where else None)

    def with_aggs(self, swap):
        """The same query with other aggregator kinds (the oracle knows sum / avg / count)."""
        c = Case.__new__(Case)
        c.name, c.stream, c.pushes = self.name, self.stream, self.pushes
        c.app = self.app
        for a, b in swap.items():
            c.app = re.sub(r"\b%s\(" % a, b + "(", c.app)
        s = self.spec
        c.spec = mm.Spec(s.window, [(swap.get(k, k), a, t) for k, a, t in s.aggs], s.outputs, s.events, s.group,
                         s.partition, s.having, s.where)
        return c


def diff(a, b):
    return None if a is None or b is None else a - b


SHAPES = [
    Case("length5-all", "length(5)", ["i", "max(x)", "min(x)"], "all"),
    Case("length5-current-long", "length(5)", ["i", "max(y)", "min(y)"]),
    Case("length5-expired-float", "length(5)", ["i", "min(f)", "max(f)"], "expired"),
    Case("length5-expired-quirk", "length(5)", ["i", "max(x)", "min(x)"], "expired", pushes=QUIRK_PUSHES),
    Case("length64-double-nulls", "length(64)", ["i", "max(d)", "min(f)", "count()"], "all", stream={"nulls": True}),
    Case("length5-special", "length(5)", ["i", "max(d)", "min(d)"], "all", stream={"special": True}),
    Case("length5-group700", "length(5)", ["g", "max(x)", "min(d)"], "all", group=True, stream={"ngroups": 700}),
    Case("length64-group-few", "length(64)", ["g", "i", "min(x)", "max(f)"], group=True, stream={"ngroups": 7}),
    Case("lengthBatch4-all", "lengthBatch(4)", ["i", "max(x)", "min(y)", "maxForever(x)", "minForever(d)"], "all"),
    Case("lengthBatch4-current-group", "lengthBatch(4)", ["g", "max(d)", "min(x)"], group=True,
         stream={"ngroups": 3}),
    Case("lengthBatch4-all-group", "lengthBatch(4)", ["g", "max(x)", "min(f)", "maxForever(d)"], "all", group=True,
         stream={"ngroups": 3}),
    Case("externalTime-all", "externalTime(et, 20)", ["i", "et", "max(x)", "min(f)"], "all"),
    Case("externalTime-group-current", "externalTime(et, 20)", ["g", "max(y)", "min(d)"], group=True,
         stream={"ngroups": 700}),
    Case("none-forever", None, ["i", "max(x)", "min(d)", "maxForever(d)", "minForever(y)"], stream={"nulls": True}),
    Case("none-group", None, ["g", "max(f)", "min(y)"], group=True, stream={"ngroups": 700}),
    Case("partition-length5", "length(5)", ["k", "i", "max(x)", "min(d)"], "all", part=True, stream={"nkeys": 5}),
    Case("partition-group-none", None, ["k", "g", "max(y)", "minForever(x)"], group=True, part=True,
         stream={"nkeys": 5, "ngroups": 40}),
    Case("five-aggregators", "length(5)", ["i", "max(x)", "min(x)", "max(d)", "sum(x)", "count()"], "all"),
    Case("having", "length(5)", ["i", "max(x)", "min(x)"], "all", having=(1, ">", 4)),
    Case("expression", "length(64)", ["i", ("max(d) - min(d)", ["max(d)", "min(d)"], diff)], "all"),
    Case("filter", "length(5)", ["i", "max(x)", "min(x)"], "all", where=("x > 1", lambda d: d[3] is not None and d[3] > 1)),
]
TO_ORACLE = {"max": "sum", "min": "avg", "maxForever": "sum", "minForever": "count"}


# ---------------------------------------------------------------- runners
def model_chunks(spec, d, pushes=PUSHES):
    m = mm.Model(spec)
    evs = as_events(d)
    out = []
    for a, b, call in pushes:
        out.extend(m.run([evs[x:min(x + call, b)] for x in range(a, b, call)]))
    return mm.norm_chunks(out)


def new_runtime(app, got, engine_factory=None):
    r = rt.SiddhiManager(engine_factory=engine_factory).createSiddhiAppRuntime(app)
    r.addCallback("q", rt._FnQueryCallback(
        lambda ts, cur, rem: got.append(([(e.timestamp, [mm.norm(x) for x in e.data]) for e in (cur or [])],
                                         [(e.timestamp, [mm.norm(x) for x in e.data]) for e in (rem or [])]))))
    r.start()
    return r


def runtime_chunks(app, d, engine_factory=None, pushes=PUSHES, snapshot_after=None):
    """Callbacks of the app over the pushes, in norm_chunks' form; with
    snapshot_after = p the state is saved after push p and the rest runs in a
    fresh runtime restored from it."""
    got = []
    r = new_runtime(app, got, engine_factory)
    for p, (a, b, call) in enumerate(pushes):
        r.getInputHandler("S").send_batch(as_batch(d, a, b, call, r.dictionary))
        if snapshot_after == p:
            image = r.snapshot()
            r.shutdown()
            r = new_runtime(app, got, engine_factory)
            r.restore(image)
    r.shutdown()
    return got


def assert_same(got, want):
    assert len(want) > 0
    for n, (a, b) in enumerate(zip(got, want)):
        assert a == b, "callback %d: got %r, the model has %r" % (n, a, b)
    assert len(got) == len(want)


# ---------------------------------------------------------------- known answers
def load_kats():
    cases = []
    for f in sorted(os.listdir(KAT_DIR)):
        if f.endswith(".json"):
            with open(os.path.join(KAT_DIR, f)) as fp:
                cases.extend(json.load(fp))
    return cases


def short(case):
    return case["name"].replace("AggregatorExtensionTestCase", "").replace("TestCase1", "")


def _forever_specs():
    out = {}
    for fn, cap in (("maxForever", "MaxForever"), ("minForever", "MinForever")):
        for n, t in ((1, mm.T_DOUBLE), (2, mm.T_INT), (3, mm.T_FLOAT), (4, mm.T_LONG)):
            out["%sAggregatorExtensionTestCase.test%sAggregatorExtension%d" % (cap, cap, n)] = \
                mm.Spec(None, [(fn, 0, t)], [("agg", 0)])
        out["%sAggregatorExtensionTestCase.%sAttributeAggregatorTest7" % (cap, fn)] = \
            mm.Spec(None, [(fn, 0, mm.T_DOUBLE)], [("agg", 0)])
    return out


KAT_SPECS = dict(_forever_specs())
KAT_SPECS["MaxAggregatorExtensionTestCase.testMaxAggregatorExtension1"] = \
    mm.Spec(("time", 1000), [("max", 0, mm.T_DOUBLE)], [("agg", 0)], "all")
for _n, _fn in ((8, "max"), (9, "min")):
    KAT_SPECS["PartitionTestCase1.testPartitionQuery%d" % _n] = \
        mm.Spec(None, [(_fn, 1, mm.T_FLOAT)], [("attr", 0), ("agg", 0), ("attr", 2)], partition=0)

KATS = load_kats()
RUN_KATS = [c for c in KATS if "expected_exception" not in c]
FAIL_KATS = [c for c in KATS if "expected_exception" in c]


class _Ev:
    def __init__(self, data):
        self.data = data

    def getData(self):  # noqa: N802
        return self.data


class _Col:
    def __init__(self):
        self.in_events, self.remove_events, self.chunks = [], [], []


def model_collector(case):
    """The case's sends through the model, collected as tests/kat_runner.py's callbacks collect."""
    m = mm.Model(KAT_SPECS[case["name"]])
    col = _Col()
    stream_cb = case["callback"]["kind"] == "stream"

    def take(chunks):
        for c in chunks:
            cur = [_Ev([None if v is None else (float(v) if isinstance(v, np.floating) else v) for v in vals])
                   for t, ts, vals in c if t == mm.CURRENT or stream_cb]
            rem = [_Ev(list(vals)) for t, ts, vals in c if t == mm.EXPIRED and not stream_cb]
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
