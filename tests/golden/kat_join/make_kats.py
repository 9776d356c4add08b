"""Writes JoinTestCase.json and OuterJoinTestCase.json: the reference's join
tests, transcribed by hand (README.md lists every test of the two files).

Format: tests/kat_runner.py's, plus `expected_chunks`, `expected_exception`
(as in ../kat_external_time_batch) and two fields of this directory:
`expected_arrived` (the reference asserts only its `eventArrived` flag) and
`not_run` (transcribed, but the library refuses the app: the reason).

The reference apps run on the wall clock and sleep between sends; here every
send carries a timestamp of a playback-style clock that starts at T0, one
millisecond per send, a `Thread.sleep(n)` adding n.  Waits after the last send
become {"time": ...} steps long enough for every window to drain.
"""
import json
import os

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = "modules/siddhi-core/src/test/java/io/siddhi/core/query/join/"
T0 = 1_000_000
STREAMS = ("define stream cseEventStream (symbol string, price float, volume int); "
           "define stream twitterStream (user string, tweet string, company string); ")
STREAMS_SYM = ("define stream cseEventStream (symbol string, price float, volume int); "
               "define stream twitterStream (user string, tweet string, symbol string); ")
Q = "@info(name = 'query1') "
SEL3 = "select cseEventStream.symbol as symbol, twitterStream.tweet, cseEventStream.price "
SEL4 = ("select cseEventStream.symbol as symbol, twitterStream.tweet, cseEventStream.price,twitterStream"
        ".company as company ")


def f(x):
    return {"float": x}


def cse(sym, price, vol):
    return ("cseEventStream", [sym, f(price), {"int": vol}])


def tw(user, tweet, company):
    return ("twitterStream", [user, tweet, company])


def sends(*steps):
    """steps: (stream, data) sends and ("sleep", ms) pauses -> kat_runner sends."""
    out, t = [], T0
    for a, b in steps:
        if a == "sleep":
            t += b
            out.append({"time": t})
        else:
            t += 1
            out.append({"stream": a, "ts": t, "data": b})
    return out


def case(cls, name, line, app, steps=(), **kw):
    c = {"name": "%s.%s" % (cls, name), "source": "%s%s.java:%d" % (SRC, cls, line), "app": app,
         "callback": {"kind": "query", "name": "query1"}, "sends": sends(*steps), "expected_rows": [],
         "expected_count": None, "expected_remove_count": None, "expected_chunk_sizes": {}, "expected_cells": [],
         "expected_nth": [], "playback": False, "start_time": T0}
    c.update(kw)
    return c


def rows(*data):
    return [{"n": i + 1, "data": list(d)} for i, d in enumerate(data)]


TIME_REASON = "time windows on a join side are refused (DESIGN.md section 7)"
W4 = [cse("WSO2", 55.6, 100), tw("User1", "Hello World", "WSO2"), cse("IBM", 75.6, 100)]

JOIN = [
    case("JoinTestCase", "joinTest1", 50,
         STREAMS + Q + "from cseEventStream#window.time(1 sec) join twitterStream#window.time(1 sec) "
         "on cseEventStream.symbol== twitterStream.company " + SEL3 + "insert all events into outputStream ;",
         W4 + [("sleep", 500), cse("WSO2", 57.6, 100), ("sleep", 2000)],
         expected_count=2, expected_remove_count=2, expected_arrived=True, not_run=TIME_REASON),
    case("JoinTestCase", "joinTest2", 99,
         STREAMS + Q + "from cseEventStream#window.time(1 sec) as a join twitterStream#window.time(1 sec) as b "
         "on a.symbol== b.company select a.symbol as symbol, b.tweet, a.price insert all events into outputStream ;",
         W4 + [("sleep", 500), cse("WSO2", 57.6, 100), ("sleep", 2000)],
         expected_count=2, expected_remove_count=2, expected_arrived=True, not_run=TIME_REASON),
    case("JoinTestCase", "joinTest4", 244,
         STREAMS + Q + "from cseEventStream#window.time(2 sec) join twitterStream#window.time(2 sec) "
         "on cseEventStream.symbol== twitterStream.company " + SEL3 + "insert all events into outputStream ;",
         W4 + [("sleep", 1000), cse("WSO2", 57.6, 100), ("sleep", 4000)],
         expected_count=2, expected_remove_count=2, expected_arrived=True, not_run=TIME_REASON),
    case("JoinTestCase", "joinTest5", 302,
         STREAMS + Q + "from cseEventStream#window.length(1) join twitterStream#window.length(1) " + SEL3 +
         "insert all events into outputStream ;",
         W4 + [cse("WSO2", 57.6, 100), ("sleep", 500)], expected_arrived=True),
    case("JoinTestCase", "joinTest6", 339,
         STREAMS_SYM + Q + "from cseEventStream join twitterStream "
         "select symbol, twitterStream.tweet, cseEventStream.price insert all events into outputStream ;",
         expected_exception="SiddhiAppValidationException"),
    case("JoinTestCase", "joinTest7", 356,
         STREAMS_SYM + Q + "from cseEventStream as a join twitterStream as b "
         "select a.symbol, twitterStream.tweet, a.price insert all events into outputStream ;",
         expected_exception="SiddhiAppValidationException"),
    case("JoinTestCase", "joinTest8", 373,
         STREAMS + Q + "from cseEventStream#window.length(1) join twitterStream#window.length(1) "
         "select cseEventStream.symbol as symbol, tweet, price insert all events into outputStream ;",
         W4 + [cse("WSO2", 57.6, 100), ("sleep", 500)], expected_arrived=True),
    case("JoinTestCase", "joinTest12", 540,
         STREAMS + Q + "from cseEventStream#window.time(1 sec) join twitterStream#window.time(1 sec) "
         "on cseEventStream.symbol== twitterStream.company select * insert into outputStream ;",
         [cse("WSO2", 55.6, 100), tw("User1", "Hello World", "WSO2"), ("sleep", 2000)],
         expected_count=1, expected_remove_count=0, expected_arrived=True, not_run=TIME_REASON),
    case("JoinTestCase", "joinTest13", 585,
         STREAMS_SYM + Q + "from cseEventStream#window.time(1 sec) join twitterStream#window.time(1 sec) "
         "on cseEventStream.symbol== twitterStream.symbol select * insert into outputStream ;",
         expected_exception="SiddhiAppValidationException"),
]

ON = "on cseEventStream.symbol== twitterStream.company "
OUTER = [
    case("OuterJoinTestCase", "joinTest1", 46,
         STREAMS + Q + "from cseEventStream#window.length(3) full outer join twitterStream#window.length(1) " + ON +
         SEL3 + "insert all events into outputStream ;",
         W4 + [cse("WSO2", 57.6, 100), ("sleep", 500)],
         expected_rows=rows(["WSO2", None, f(55.6)], ["WSO2", "Hello World", f(55.6)], ["IBM", None, f(75.6)],
                            ["WSO2", "Hello World", f(57.6)]),
         expected_count=4, expected_arrived=True),
    case("OuterJoinTestCase", "joinTest2", 106,
         STREAMS + Q + "from cseEventStream#window.length(1) right outer join twitterStream#window.length(2) " + ON +
         SEL4 + "insert all events into outputStream ;",
         [tw("User1", "Hello World", "WSO2"), cse("BMW", 57.6, 100), tw("User2", "Welcome", "IBM"),
          cse("WSO2", 57.6, 100), ("sleep", 500)],
         expected_rows=rows([None, "Hello World", None, "WSO2"], [None, "Welcome", None, "IBM"],
                            ["WSO2", "Hello World", f(57.6), "WSO2"]),
         expected_count=3, expected_arrived=True),
    case("OuterJoinTestCase", "joinTest3", 166,
         STREAMS + Q + "from cseEventStream#window.length(2) left outer join twitterStream#window.length(1) " + ON +
         SEL4 + "insert all events into outputStream ;",
         [cse("WSO2", 57.6, 100), tw("User2", "Welcome", "BMW"), cse("IBM", 47.6, 200),
          tw("User1", "Hello World", "WSO2"), ("sleep", 500)],
         expected_rows=rows(["WSO2", None, f(57.6), None], ["IBM", None, f(47.6), None],
                            ["WSO2", "Hello World", f(57.6), "WSO2"]),
         expected_count=3, expected_arrived=True),
    case("OuterJoinTestCase", "joinTest4", 226,
         STREAMS_SYM + Q + "from cseEventStream#window.time(1 sec) outer join twitterStream#window.time(1 sec) "
         "on cseEventStream.symbol== twitterStream.symbol select * insert into outputStream ;",
         expected_exception="SiddhiParserException"),
    case("OuterJoinTestCase", "joinTest5", 246,
         STREAMS_SYM + Q + "from cseEventStream#window.time(1 sec) full outer join twitterStream#window.time(1 sec) "
         "on cseEventStream.symbol== twitterStream.symbol select * insert into outputStream ;",
         expected_exception="SiddhiAppValidationException"),
    case("OuterJoinTestCase", "joinTest6", 266,
         STREAMS + Q + "from cseEventStream#window.length(2) right outer join twitterStream " + ON +
         "select cseEventStream.symbol as symbol, twitterStream.tweet insert all events into outputStream ;",
         [cse("IBM", 57.6, 100), cse("WSO2", 57.6, 100), ("sleep", 500)], expected_arrived=False),
    case("OuterJoinTestCase", "joinTest7", 300,
         STREAMS + Q + "from cseEventStream left outer join twitterStream#window.length(2) " + ON +
         "select cseEventStream.symbol as symbol, twitterStream.tweet insert all events into outputStream ;",
         [tw("User2", "Welcome", "BMW"), tw("User1", "Hello World", "WSO2"), ("sleep", 500)],
         expected_arrived=False),
    case("OuterJoinTestCase", "joinTest8", 333,
         STREAMS + Q + "from cseEventStream#window.length(3) inner join twitterStream#window.length(1) " + ON + SEL3 +
         "insert all events into outputStream ;",
         [cse("WSO2", 55.6, 100), tw("User", "Hello World", "WSO2"), cse("IBM", 75.6, 100), ("sleep", 500),
          cse("WSO2", 57.6, 100), ("sleep", 2000)],
         expected_rows=rows(["WSO2", "Hello World", f(55.6)], ["WSO2", "Hello World", f(57.6)]),
         expected_count=2, expected_arrived=True),
    case("OuterJoinTestCase", "joinTest9", 385,
         STREAMS + Q + "from cseEventStream#window.length(3) join twitterStream#window.length(1) " + ON + SEL3 +
         "insert all events into outputStream ;",
         [cse("WSO2", 55.6, 100), tw("User", "Hello World", "BMW"), cse("IBM", 75.6, 100), cse("WSO2", 57.6, 100),
          ("sleep", 500)], expected_arrived=False),
]

if __name__ == "__main__":
    for name, cases in (("JoinTestCase", JOIN), ("OuterJoinTestCase", OUTER)):
        with open(os.path.join(HERE, name + ".json"), "w") as fp:
            json.dump(cases, fp, indent=1)
            fp.write("\n")
