"""Stream-stream window joins on the CPU: the Python model (tests/join_model.py)
against the reference's own known answers, the parser's and planner's lowering
of every supported form, and every refusal (DESIGN.md "Joins", section 7).
"""
import json
import os
import re
import shutil
import subprocess

import pytest

import join_cases as jc
import join_model as jm
from kat_runner import check_case
from siddhi_amd import planner as pl
from siddhi_amd import query_compiler as qc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AB = "define stream A (k int, price float, id long); define stream B (k int, lim float, id long); "


def plan_of(text, query=0):
    app = qc.parse(text)
    items = []
    for it in app.execution_order:
        items.extend([(q, it) for q in it.queries] if isinstance(it, qc.Partition) else [(it, None)])
    q, part = items[query]
    return pl.plan_query(app, q, pl.StringDictionary(), part)


# ---------------------------------------------------------------- known answers
def test_every_transcribed_case_has_a_spec():
    assert sorted(jc.SPECS) == sorted(jc.short(c) for c in jc.MODEL_CASES)
    assert len(jc.RUN_CASES) == 9 and len(jc.REFUSED_CASES) == 4 and len(jc.FAIL_CASES) == 5


@pytest.mark.parametrize("case", jc.MODEL_CASES, ids=[jc.short(c) for c in jc.MODEL_CASES])
def test_model_reproduces_reference_known_answer(case):
    """Validates the model (the time cases too), not the feature."""
    col = jc.model_collector(case)
    errs = check_case(case, col) + jc.check_extras(case, col)
    assert not errs, "%s (%s): %s" % (case["name"], case["source"], errs)


@pytest.mark.parametrize("case", jc.RUN_CASES, ids=[jc.short(c) for c in jc.RUN_CASES])
def test_transcribed_case_plans_as_a_join(case):
    qp = plan_of(case["app"])
    assert qp.plan.kind == pl.KIND_JOIN and len(qp.input_streams) == 2


@pytest.mark.parametrize("case", jc.FAIL_CASES, ids=[jc.short(c) for c in jc.FAIL_CASES])
def test_reference_creation_failures(case):
    exc = {"SiddhiAppValidationException": pl.SiddhiAppValidationException,
           "SiddhiParserException": qc.SiddhiParserException}[case["expected_exception"]]
    with pytest.raises(exc) as ei:
        plan_of(case["app"])
    assert not isinstance(ei.value, (pl.UnsupportedPlanException, qc.OutOfScopeSyntax))


@pytest.mark.parametrize("case", jc.REFUSED_CASES, ids=[jc.short(c) for c in jc.REFUSED_CASES])
def test_time_cases_are_refused(case):
    with pytest.raises(pl.UnsupportedPlanException, match="time windows on a join side"):
        plan_of(case["app"])


# ---------------------------------------------------------------- parser and planner
def test_parser_builds_a_join_input():
    app = qc.parse(AB + "from A[price > 1]#window.length(3) as a unidirectional left outer join "
                   "B#window.length(1) as b on a.k == b.k and a.price > b.lim select a.k as ak, b.lim "
                   "insert all events into O;")
    ji = app.queries[0].input
    assert isinstance(ji, qc.JoinInput)
    assert (ji.left.stream, ji.left.ref, ji.right.stream, ji.right.ref) == ("A", "a", "B", "b")
    assert ji.type == "left_outer" and ji.left_unidirectional and not ji.right_unidirectional
    assert isinstance(ji.on, qc.BinOp) and ji.on.op == "and"
    assert [type(h).__name__ for h in ji.left.handlers] == ["Filter", "Window"]


FORMS = [
    ("join", "inner", (True, True), (False, False)),
    ("inner join", "inner", (True, True), (False, False)),
    ("left outer join", "left_outer", (True, True), (True, False)),
    ("right outer join", "right_outer", (True, True), (False, True)),
    ("full outer join", "full_outer", (True, True), (True, True)),
]


@pytest.mark.parametrize("words,kind,trigger,outer", FORMS, ids=[f[0] for f in FORMS])
def test_join_types_lower_to_flags(words, kind, trigger, outer):
    qp = plan_of(AB + "from A#window.length(5) as a %s B#window.length(2) as b on a.k == b.k "
                 "select a.id as aid, b.id as bid insert into O;" % words)
    p = qp.plan
    assert p.kind == pl.KIND_JOIN and p.join_type == pl.JOIN_TYPES[kind]
    assert [(s[1], s[2]) for s in p.join_sides] == list(zip(trigger, outer))
    assert [(s[0], s[3], s[4]) for s in p.join_sides] == [(0, pl.W_LENGTH, 5), (1, pl.W_LENGTH, 2)]
    assert qp.input_streams == ["A", "B"] and qp.output_names == ["aid", "bid"]
    assert p.join_on >= 0 and p.current_on and not p.expired_on


def test_unidirectional_and_windowless_sides():
    p = plan_of(AB + "from A as a unidirectional join B#window.length(2) as b select a.id as aid, b.id as bid "
                "insert expired events into O;").plan
    assert [(s[1], s[3]) for s in p.join_sides] == [(True, 0), (False, pl.W_LENGTH)]
    assert p.join_on == -1 and p.expired_on and not p.current_on
    p = plan_of(AB + "from A#window.length(1) join B[lim > 2.0] unidirectional on A.k == B.k "
                "select A.id as aid, B.id as bid insert into O;").plan
    assert [(s[1], s[3], len(s[5])) for s in p.join_sides] == [(False, pl.W_LENGTH, 0), (True, 0, 1)]


def test_operands_are_addressed_by_side():
    p = plan_of(AB + "from A[price > 1.0]#window.length(3) as a join B[lim < 9.0]#window.length(3) as b "
                "on a.price > b.lim select a.k as ak, b.k as bk insert into O;").plan
    loads = lambda e: [(i[1], i[3] & 0xFFFF) for i in p.exprs[e] if i[0] == pl.OP_LOAD]
    assert loads(p.join_sides[0][5][0]) == [(0, 1)] and loads(p.join_sides[1][5][0]) == [(1, 1)]
    assert loads(p.join_on) == [(0, 1), (1, 1)]
    assert [loads(e) for _, _, e in p.outputs] == [[(0, 0)], [(1, 0)]]


def test_join_plan_bytes_and_old_encodings():
    """A join plan is kind 3 under the unchanged IR version (a single-stream
    plan still kind 2), laid out as include/siddhi_ir.h says."""
    qp = plan_of(AB + "from A#window.length(2) join B on A.k == B.k select A.id as aid insert into O;")
    w = qp.plan.to_words()
    assert w[:3] == [pl.MAGIC, 1, 3] and pl.VERSION == 1
    single = plan_of(AB + "from A#window.length(2) select id insert into O;").plan.to_words()
    assert single[:3] == [pl.MAGIC, 1, 2]
    # two streams of three attributes each (int, float, long), no constants
    assert w[3:13] == [2, 3, 1, 3, 2, 3, 1, 3, 2, 0]
    # the join section -- type, { stream, trigger, outer, window, p_lo, p_hi, n_filters } * 2, on -- then the
    # selector: current-only, no aggregators, group by or having, one LONG output; then the null-string id
    join = [0, 0, 1, 0, pl.W_LENGTH, 2, 0, 0, 1, 1, 0, 0, 0, 0, 0, qp.plan.join_on]
    selector = [1, 0, 0, 0, -1, 1, pl.T_LONG, qp.plan.outputs[0][2], -1, -1]
    assert w[-len(join + selector):] == join + selector


# ---------------------------------------------------------------- refusals
J = "from A#window.length(2) as a join B#window.length(2) as b on a.k == b.k "
REFUSALS = [
    ("aggregating selector", AB + J + "select count() as n insert into O;", "aggregating selectors over a join"),
    ("group by", AB + J + "select a.k as ak group by a.k insert into O;", "group by over a join"),
    ("having", AB + J + "select a.k as ak having ak > 1 insert into O;", "having over a join"),
    ("partition", AB + "partition with (k of A, k of B) begin " + J + "select a.id as aid insert into O; end;",
     "joins inside a partition"),
    ("self-join", AB + "from A#window.length(2) as a join A#window.length(2) as b on a.k == b.k "
     "select a.id as aid insert into O;", "self-joins"),
    ("lengthBatch side", AB + "from A#window.lengthBatch(2) as a join B as b select a.id as aid insert into O;",
     "window lengthbatch on a join side"),
    ("timeBatch side", AB + "from A as a join B#window.timeBatch(1 sec) as b select a.id as aid insert into O;",
     "window timebatch on a join side"),
    ("time side", AB + "from A#window.time(1 sec) as a join B as b select a.id as aid insert into O;",
     "time windows on a join side"),
    ("length(0) side", AB + "from A#window.length(0) as a join B as b select a.id as aid insert into O;",
     r"length\(0\) on a join side"),
    ("within / per", AB + "from A as a join B as b on a.k == b.k within 1, 2 per 'days' "
     "select a.id as aid insert into O;", "within"),
    ("output rate", AB + J + "select a.id as aid output every 2 events insert into O;",
     "output rate limiting on a join"),
]


@pytest.mark.parametrize("name,text,message", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refused_with_unsupported_plan(name, text, message):
    with pytest.raises(pl.UnsupportedPlanException, match=message):
        plan_of(text)


def test_a_side_that_is_no_defined_stream_is_refused():
    """Tables, named windows and aggregations have no definition here."""
    app = qc.parse(AB + J + "select a.id as aid insert into O;")
    app.queries[0].input.right.stream = "SomeTable"
    with pytest.raises(pl.UnsupportedPlanException, match="tables, named windows and aggregations"):
        pl.plan_query(app, app.queries[0], pl.StringDictionary())


VALIDATION = [
    ("ambiguous attribute", AB + "from A#window.length(1) join B#window.length(1) select k insert into O;"),
    ("ambiguous in on", AB + "from A#window.length(1) join B#window.length(1) on k == 1 select A.id as i "
     "insert into O;"),
    ("stream id despite alias", AB + "from A as a join B as b select a.id as i, B.lim as l insert into O;"),
    ("both unidirectional", AB + "from A unidirectional join B unidirectional select A.id as i insert into O;"),
]


@pytest.mark.parametrize("name,text", VALIDATION, ids=[v[0] for v in VALIDATION])
def test_refused_with_validation_exception(name, text):
    with pytest.raises(pl.SiddhiAppValidationException) as ei:
        plan_of(text)
    assert not isinstance(ei.value, pl.UnsupportedPlanException)


def test_length_batch_join_cases_of_the_window_kat_still_refuse():
    with open(os.path.join(ROOT, "tests", "golden", "kat", "LengthBatchWindowTestCase.json")) as fp:
        cases = [c for c in json.load(fp) if " join " in c["app"]]
    assert len(cases) == 4
    for c in cases:
        with pytest.raises(pl.UnsupportedPlanException):
            plan_of(c["app"])


# ---------------------------------------------------------------- the model itself
def test_model_length_chunk_order_and_outer_rows():
    """length(1) left side, all events: the pushed-out event triggers before
    the one that pushed it out; both carry the clock / their own timestamp."""
    spec = jm.Spec(jm.Side(("length", 1)), jm.Side(("length", 2)), lambda l, r: [l and l[0], r and r[0]],
                   lambda l, r: l[0] == r[0], "full_outer", "all")
    m = jm.Model(spec)
    assert m.send(1, [(10, [1])]) == [(jm.CURRENT, 10, [None, 1])]
    assert m.send(0, [(11, [1])]) == [(jm.CURRENT, 11, [1, 1])]
    assert m.send(0, [(12, [2]), (15, [1])]) == [(jm.EXPIRED, 15, [1, 1]), (jm.CURRENT, 12, [2, None]),
                                                 (jm.EXPIRED, 15, [2, None]), (jm.CURRENT, 15, [1, 1])]


def test_model_windowless_side_triggers_but_is_never_found():
    spec = jm.Spec(jm.Side(None), jm.Side(("length", 2)), lambda l, r: [l and l[0], r and r[0]], None, "inner", "all")
    m = jm.Model(spec)
    assert m.send(0, [(1, [7])]) is None
    assert m.send(1, [(2, [8])]) is None
    assert m.send(0, [(3, [9])]) == [(jm.CURRENT, 3, [9, 8]), (jm.EXPIRED, 3, [9, 8])]


# ---------------------------------------------------------------- kernel constants
def test_tile_numbers_match_the_kernel_source():
    with open(os.path.join(ROOT, "siddhi_amd", "csrc", "engine_join.hip")) as fp:
        src = fp.read()
    trig = re.search(r"constexpr int kJoinTrig = (\d+);", src)
    tile = re.search(r"constexpr int kJoinTile = (\d+);", src)
    assert trig and tile
    assert (int(trig.group(1)), int(tile.group(1))) == (jc.JOIN_TRIG, jc.JOIN_TILE)


def test_join_kernels_keep_the_device_code_rules(tmp_path):
    """tests/test_kernel_isa.py's checks on engine_join.hip's gfx950 assembly: no
    vector access to the kernarg segment, no scratch in the join kernels, and
    the LDS of one workgroup as DESIGN.md states it (one tile: 9 KiB and change)."""
    from isa_check import scan
    csrc = os.path.join(ROOT, "siddhi_amd", "csrc")
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    asm = str(tmp_path / "engine_join.s")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-x", "hip",
                           "--cuda-device-only", "-S", os.path.join(csrc, "engine_join.hip"), "-o", asm],
                          stderr=subprocess.DEVNULL)
    assert not scan(asm)
    text = open(asm).read()
    meta = re.findall(r"\.group_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.name:\s+(\S+)\n(?:.*\n)*?"
                      r"\s+\.private_segment_fixed_size:\s+(\d+)", text)
    join = [(name, int(lds), int(priv)) for lds, name, priv in meta if "k_join_" in name]
    assert sorted(n.split("k_join_")[1][:5] for n, _, _ in join) == ["carry", "count", "emitE", "total"]
    for name, lds, priv in join:
        assert priv == 0, "%s uses %d bytes of scratch" % (name, priv)
        assert lds <= 16 * jc.JOIN_TILE * 9 + 64, "%s: %d bytes of LDS" % (name, lds)
