"""Writes the known-answer files of this directory.  Every case is the
reference's own test, transcribed by hand (README.md): app, sends, the rows the
test asserts and the line it starts at.  Run from anywhere: python make_kats.py
"""
import json
import os

HERE = os.path.dirname(os.path.abspath(__file__))
T = "modules/siddhi-core/src/test/java/io/siddhi/core/query/"
CLOCK0 = 1_000_000
# StdDevAttributeAggregatorExecutorTestCase.java:36: `private final double epsilon = 0.00001`;
# every stdDev assertion there is Math.abs(expected - actual) < epsilon
EPSILON = 0.00001


def case(name, source, app, callback, steps, rows=None, count=None, exception=None, note=None, epsilon=None):
    """steps: a list of (stream, data) sends, each one millisecond after the
    last, and ("sleep", ms) pauses."""
    clock = CLOCK0
    sends = []
    for s in steps:
        if s[0] == "sleep":
            clock += s[1]
            sends.append({"time": clock})
        else:
            clock += 1
            sends.append({"stream": s[0], "ts": clock, "data": s[1]})
    c = {"name": name, "source": T + source, "app": app, "callback": callback, "sends": sends}
    if exception:
        c["expected_exception"] = exception
    else:
        c["expected_count"] = count
        c["expected_rows"] = [{"n": n + 1, "data": r} for n, r in enumerate(rows)]
    if epsilon is not None:
        c["epsilon"] = epsilon
    if note:
        c["note"] = note
    return c


Q1 = {"kind": "query", "name": "query1"}
OUT = {"kind": "stream", "name": "outputStream"}


def stddev():
    src = "selector/attribute/aggregator/StdDevAttributeAggregatorExecutorTestCase.java:%d"
    name = "StdDevAttributeAggregatorExecutorTestCase.stdDevAggregatorTest%d"
    head = "@app:name('stdDevAggregatorTests') define stream cseEventStream (symbol string, price double);" \
           "@info(name = 'query1') from cseEventStream%s select stdDev(price) as deviation group by symbol " \
           "insert %sinto outputStream;"

    def sends(rows):
        return [("cseEventStream", list(r)) for r in rows]

    return [
        case(name % 1, src % 46, head % ("", ""), Q1, [("sleep", 10)], [], 0, epsilon=EPSILON),
        case(name % 2, src % 82, head % ("#window.lengthBatch(1)", ""), Q1, sends([("WSO2", 1.0)]) + [("sleep", 100)],
             [[0.0]], 1, epsilon=EPSILON),
        case(name % 3, src % 118, head % ("#window.lengthBatch(3)", ""), Q1,
             sends([("WSO2", 1.0)] * 3) + [("sleep", 300)], [[0.0]], 1, epsilon=EPSILON),
        case(name % 4, src % 156, head % ("#window.lengthBatch(6)", ""), Q1,
             sends([("WSO2", 10000.0), ("WSO2", 10000.5), ("WSO2", 10001.0), ("IBM", 1.0), ("IBM", 1.5), ("IBM", 2.0)])
             + [("sleep", 600)], [[0.40825], [0.40825]], 2, epsilon=EPSILON),
        case(name % 5, src % 198, head % ("#window.lengthBatch(6)", ""), Q1,
             sends([("WSO2", 23.0), ("WSO2", 1003.0), ("WSO2", 500.0), ("IBM", 0.002), ("IBM", 0.0034),
                    ("IBM", 0.00454)]) + [("sleep", 600)], [[400.13025], [0.00103]], 2, epsilon=EPSILON),
        case(name % 6, src % 240, head % ("#window.length(3)", "all events "), Q1,
             [s for p in (23.3, 1003.2, 500.1, 10.9, 234.5) for s in (("cseEventStream", ["WSO2", p]), ("sleep", 100))],
             [[0.0], [489.95], [400.09052], [405.11802], [199.96026]], 5, epsilon=EPSILON),
        case(name % 8, src % 289,
             "define stream cseEventStream (symbol string, price double, discount int);@info(name = 'query1') "
             "from cseEventStream#window.lengthBatch(1) select stdDev(price, discount) as deviation group by symbol "
             "insert into outputStream;", Q1, [], exception="SiddhiAppCreationException"),
    ]


def distinct():
    src = "selector/attribute/aggregator/DistinctCountAttributeAggregatorExecutorTestCase.java:%d"
    app = "define stream inputStream (eventId string, userID string, pageID string); @info(name = 'query1') " \
          "from inputStream#window.time(5 sec) select userID, pageID, %s as distinctPages group by userID " \
          "having distinctPages > 3 insert into outputStream; "
    rows = [("E001", "USER_1", "WEB_PAGE_1"), ("E002", "USER_2", "WEB_PAGE_1"), ("E003", "USER_1", "WEB_PAGE_2"),
            ("E004", "USER_2", "WEB_PAGE_2"), ("E005", "USER_1", "WEB_PAGE_3"), ("E006", "USER_1", "WEB_PAGE_1"),
            ("E007", "USER_1", "WEB_PAGE_4"), ("E008", "USER_2", "WEB_PAGE_2"), ("E009", "USER_1", "WEB_PAGE_1"),
            ("E010", "USER_2", "WEB_PAGE_1")]
    steps = []
    for n, r in enumerate(rows):
        steps.append(("inputStream", list(r)))
        steps.append(("sleep", 2000 if n == len(rows) - 1 else 1000))
    return [
        case("DistinctCountAttributeAggregatorExecutorTestCase.distinctCountTest", src % 44,
             app % "distinctCount(pageID)", OUT, steps, [["USER_1", "WEB_PAGE_4", {"long": 4}]], 1),
        case("DistinctCountAttributeAggregatorExecutorTestCase.distinctCountTest2", src % 104,
             app % "distinctCount()", OUT, steps, exception="SiddhiAppCreationException"),
    ]


def logical(cap, fn, lines, more_name, more_sends, rows):
    """rows: the isValidTransaction each scenario asserts, event by event."""
    src = "aggregator/%sAggregatorExtensionTestCase.java:%%d" % cap
    app = "define stream cscStream(messageID string, isFraud bool, price double);@info(name = 'query1') " \
          "from cscStream#window.lengthBatch(%%d) select messageID, %s(isFraud) as isValidTransaction " \
          "group by messageID insert all events into outputStream;" % fn
    plain = "@app:name('%sAggregatorTests') define stream cseEventStream (name string, isFraud bool);" \
            "@info(name = 'query1') from cseEventStream select %s(isFraud) as isFraudTransaction " \
            "insert into outputStream;" % (fn, fn)

    def sends(flags):
        return [("cscStream", ["messageId1", b, 35.75]) for b in flags]

    name = "%sAggregatorExtensionTestCase." % cap
    scen = "test%sAggregator%%sScenario" % cap
    return [
        case(name + scen % "TrueOnly", src % lines[0], app % 3, OUT, sends([True] * 3) + [("sleep", 2000)],
             [["messageId1", rows[0]]], 1),
        case(name + scen % "FalseOnly", src % lines[1], app % 4, OUT, sends([False] * 4) + [("sleep", 2000)],
             [["messageId1", rows[1]]], 1),
        case(name + scen % "TrueFalse", src % lines[2], app % 4, OUT,
             sends([False, True, False, True]) + [("sleep", 2000)], [["messageId1", rows[2]]], 1),
        case(name + more_name, src % lines[3], app % 2, OUT, sends(more_sends) + [("sleep", 2000)],
             [["messageId1", rows[3]], ["messageId1", rows[4]]], 2),
        case(name + "%sAggregatorTest%d" % (fn, 5 if fn == "and" else 1), src % lines[4],
             "define stream cseEventStream (name string, isFraud bool);@info(name = 'query1') "
             "from cseEventStream#window.lengthBatch(1) select %s(isFraud, name) as isFraudTransaction "
             "insert into outputStream;" % fn, Q1, [], exception="SiddhiAppCreationException"),
        case(name + "%sAggregatorTest%d" % (fn, 6 if fn == "and" else 2), src % lines[5], plain, Q1, [("sleep", 10)],
             [], 0),
    ]


def main():
    andc = logical("And", "and", [49, 97, 145, 193, 244, 259], "testAndAggregatorMoreEventsBatchScenario",
                   [False, True, True, True], [True, False, False, False, True])
    orc = logical("Or", "or", [49, 97, 145, 195, 246, 261], "testORAggregatorMoreEventsBatchScenario",
                  [False, False, True, True], [True, False, True, False, True])
    orc.append(case("OrAggregatorExtensionTestCase.orAggregatorTest3", "aggregator/OrAggregatorExtensionTestCase.java:296",
                    "@app:name('orAggregatorTests') define stream cseEventStream (name string, isFraud bool);"
                    "@info(name = 'query1') from cseEventStream select or(isFraud) as isFraudTransaction "
                    "insert into outputStream;", Q1,
                    [("cseEventStream", ["Ms1", True]), ("cseEventStream", ["Ms2", False]), ("sleep", 100)],
                    [[True], [True]], 2))
    files = {
        "StdDevAttributeAggregatorExecutorTestCase.json": stddev(),
        "DistinctCountAttributeAggregatorExecutorTestCase.json": distinct(),
        "AndAggregatorExtensionTestCase.json": andc,
        "OrAggregatorExtensionTestCase.json": orc,
    }
    for name, cases in files.items():
        with open(os.path.join(HERE, name), "w") as fp:
            json.dump(cases, fp, indent=1)
            fp.write("\n")


if __name__ == "__main__":
    main()
