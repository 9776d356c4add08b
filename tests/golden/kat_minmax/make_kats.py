"""Writes the known-answer files of this directory.  Every case is the
reference's own test, transcribed by hand (README.md): app, sends, the rows the
test asserts and the line it starts at.  Run from anywhere: python make_kats.py
"""
import json
import os

HERE = os.path.dirname(os.path.abspath(__file__))
T = "modules/siddhi-core/src/test/java/io/siddhi/core/query/"
CLOCK0 = 1_000_000


def f(x):
    return {"float": x}


def i(x):
    return {"int": x}


def lg(x):
    return {"long": x}


def case(name, source, app, callback, steps, rows=None, count=None, exception=None, note=None):
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
    if note:
        c["note"] = note
    return c


Q1 = {"kind": "query", "name": "query1"}
DD = "define stream inputStream (price1 double,price2 double, price3 double);"
PRICES = [[36.0, 36.75, 35.75], [37.88, 38.12, 37.62], [39.00, 39.25, 38.62], [36.88, 37.75, 36.75],
          [38.12, 38.12, 37.75], [38.12, 40.0, 37.75]]
INTS = [[36, 38, 74], [78, 38, 37], [9, 39, 38]]


def forever(which, col_rows_double, col_rows_int, file, lines):
    fn = which + "Forever"
    Cap = which.capitalize()
    sel = "select %s(price1) as %sValue insert into outputStream;" % (fn, fn)
    out = []
    out.append(case("%sForeverAggregatorExtensionTestCase.test%sForeverAggregatorExtension1" % (Cap, Cap),
                    "%s:%d" % (file, lines[0]), DD + "@info(name = 'query1') from inputStream " + sel, Q1,
                    [("inputStream", p) for p in PRICES] + [("sleep", 300)], [[v] for v in col_rows_double], 6))
    out.append(case("%sForeverAggregatorExtensionTestCase.test%sForeverAggregatorExtension2" % (Cap, Cap),
                    "%s:%d" % (file, lines[1]),
                    "define stream inputStream (price1 int,price2 int, price3 int);@info(name = 'query1') "
                    "from inputStream " + sel, Q1,
                    [("inputStream", [i(v) for v in r]) for r in INTS] + [("sleep", 300)],
                    [[i(v)] for v in col_rows_int], 3))
    out.append(case("%sForeverAggregatorExtensionTestCase.test%sForeverAggregatorExtension3" % (Cap, Cap),
                    "%s:%d" % (file, lines[2]),
                    "define stream inputStream (price1 float, price2 float, price3 float);@info(name = 'query1') "
                    "from inputStream " + sel, Q1,
                    [("inputStream", [f(v) for v in p]) for p in PRICES] + [("sleep", 300)],
                    [[f(v)] for v in col_rows_double], 6))
    out.append(case("%sForeverAggregatorExtensionTestCase.test%sForeverAggregatorExtension4" % (Cap, Cap),
                    "%s:%d" % (file, lines[3]),
                    "define stream inputStream (price1 long, price2 long, price3 long);@info(name = 'query1') "
                    "from inputStream select %s(price1) as %s insert into outputStream;" % (fn, fn), Q1,
                    [("inputStream", [lg(v) for v in r]) for r in INTS] + [("sleep", 300)],
                    [[lg(v)] for v in col_rows_int], 3))
    out.append(case("%sForeverAggregatorExtensionTestCase.test%sForeverAggregatorExtension5" % (Cap, Cap),
                    "%s:%d" % (file, lines[4]),
                    "define stream inputStream (price1 int,price2 double, price3 double);@info(name = 'query1') "
                    "from inputStream select %s(price1, price2, price3) as %sValue insert into outputStream;"
                    % (fn, fn), Q1, [], exception="SiddhiAppCreationException"))
    second = [30.0, 30.88, 20.0] if which == "max" else [10.0, 20.0, 25.0]
    first = [None, 20.0, 20.0] if which == "max" else [None, 20.0, None]
    out.append(case("%sForeverAggregatorExtensionTestCase.%sForeverAttributeAggregatorTest7" % (Cap, which),
                    "%s:%d" % (file, lines[5]),
                    "@app:name('%sForeverAttributeAggregatorTests') define stream cseEventStream (price1 double, "
                    "price2 double, price3 double);@info(name = 'query1') from cseEventStream "
                    "select %s(price1) as max insert into outputStream;" % (which, fn), Q1,
                    [("cseEventStream", first), ("cseEventStream", second), ("sleep", 100)],
                    [[None], [second[0]]], 2,
                    note="the reference's callback asserts inEvents[1] of one-event callbacks, which never "
                         "holds an event: the rows here are what its two sends produce (a null argument "
                         "leaves the state alone)"))
    return out


def main():
    box = [("cseEventStream", [w, "Box%d" % (n + 1)]) for n, w in enumerate([20.0, 30.0, 10.0, 40.0, 50.0])]
    bad = ("@app:name('%sAttributeAggregatorTests') define stream cseEventStream (weight double, deviceId string);"
           "@info(name = 'query1') from cseEventStream#window.lengthBatch(5) select %s(weight, deviceId) as max "
           "insert into outputStream;")
    maxc = [
        case("MaxAggregatorExtensionTestCase.testMaxAggregatorExtension1", "aggregator/MaxAggregatorExtensionTestCase.java:48",
             DD + "@info(name = 'query1') from inputStream#window.time(1 sec) select max(price1) as maxForeverValue "
             "insert all events into outputStream;", {"kind": "stream", "name": "outputStream"},
             [("inputStream", PRICES[0]), ("sleep", 100), ("inputStream", PRICES[1]), ("sleep", 2000), ("sleep", 300)],
             [[36.0], [37.88], [37.88], [None]], 4),
        case("MaxAggregatorExtensionTestCase.maxAttributeAggregatorTest2", "aggregator/MaxAggregatorExtensionTestCase.java:106",
             bad % ("max", "max"), Q1, box, exception="SiddhiAppCreationException"),
        case("MaxAggregatorExtensionTestCase.minAttributeAggregatorTest2", "aggregator/MaxAggregatorExtensionTestCase.java:145",
             bad % ("min", "min"), Q1, box, exception="SiddhiAppCreationException"),
    ]
    part = []
    stocks = [["IBM", f(75.0), i(100)], ["WSO2", f(705.0), i(100)], ["IBM", f(35.0), i(100)], ["ORACLE", f(50.0), i(100)]]
    for n, fn, line, third in ((8, "max", 631, 75.0), (9, "min", 678, 35.0)):
        part.append(case("PartitionTestCase1.testPartitionQuery%d" % n, "partition/PartitionTestCase1.java:%d" % line,
                         "@app:name('PartitionTest%d') define stream cseEventStream (symbol string, price float,volume int);"
                         "define stream cseEventStream1 (symbol string, price float,volume int);"
                         "partition with (symbol of cseEventStream) begin @info(name = 'query') from cseEventStream "
                         "select symbol,%s(price) as %s_price,volume insert into OutStockStream ;end " % (n, fn, fn),
                         {"kind": "stream", "name": "OutStockStream"},
                         [("cseEventStream", s) for s in stocks] + [("sleep", 100)],
                         [["IBM", f(75.0), i(100)], ["WSO2", f(705.0), i(100)], ["IBM", f(third), i(100)],
                          ["ORACLE", f(50.0), i(100)]], 4))
    files = {
        "MaxAggregatorExtensionTestCase.json": maxc,
        "MaxForeverAggregatorExtensionTestCase.json": forever(
            "max", [36.0, 37.88, 39.0, 39.0, 39.0, 39.0], [36, 78, 78],
            "aggregator/MaxForeverAggregatorExtensionTestCase.java", [47, 112, 164, 228, 280, 294]),
        "MinForeverAggregatorExtensionTestCase.json": forever(
            "min", [36.0] * 6, [36, 36, 9],
            "aggregator/MinForeverAggregatorExtensionTestCase.java", [47, 111, 163, 227, 279, 293]),
        "PartitionTestCase1.json": part,
    }
    for name, cases in files.items():
        with open(os.path.join(HERE, name), "w") as fp:
            json.dump(cases, fp, indent=1)
            fp.write("\n")


if __name__ == "__main__":
    main()
