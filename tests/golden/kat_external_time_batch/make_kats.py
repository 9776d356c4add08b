"""Writes ExternalTimeBatchWindowTestCase.json: the reference's timeout-free
externalTimeBatch tests (modules/siddhi-core/src/test/java/io/siddhi/core/query/
window/ExternalTimeBatchWindowTestCase.java) transcribed by hand into the case
format tests/kat_runner.py reads.  Apps, sent events and asserted values are
the reference's; Thread.sleep calls are dropped (without a timeout the window
has no clock of its own).  See README.md for what is not transcribed.

    python tests/golden/kat_external_time_batch/make_kats.py
"""
import json
import os

SRC = "modules/siddhi-core/src/test/java/io/siddhi/core/query/window/ExternalTimeBatchWindowTestCase.java:%d"
T0 = 1500000000000   # the app clock at start(); the window never reads it


def L(v):
    return {"long": v}


def I(v):
    return {"int": v}


def D(v):
    return {"double": v}


def case(name, line, app, cb, stream, events, **expect):
    c = {"name": "ExternalTimeBatchWindowTestCase." + name, "source": SRC % line, "app": app,
         "callback": {"kind": "query", "name": cb},
         "sends": [{"stream": stream, "ts": T0 + i, "data": d} for i, d in enumerate(events)],
         "expected_rows": [], "expected_count": None, "expected_remove_count": None, "expected_chunk_sizes": {},
         "expected_cells": [], "expected_nth": [], "playback": False, "start_time": T0}
    c.update(expect)
    return c


def failure(name, line, app):
    return case(name, line, app, "query1", "LoginEvents", [], expected_exception="SiddhiAppCreationException")


JMX = ("define stream jmxMetric(cpu int, timestamp long); @info(name='query')"
       "from jmxMetric#window.externalTimeBatch(timestamp, 10 sec) "
       "select avg(cpu) as avgCpu, count() as count insert into tmp;")
LOGIN = "define stream LoginEvents (timestamp long, ip string) ;"


def login(window, events="all events "):
    return (LOGIN + "@info(name = 'query1') from LoginEvents#window.externalTimeBatch(%s) "
            "select timestamp, ip, count() as total  insert %sinto uniqueIps ;" % (window, events))


def login_events(*rows):
    return [[L(1366335800000 + t), ip] for t, ip in rows]


SIX = [(4341, "192.10.1.3"), (4342, "192.10.1.4"), (5340, "192.10.1.4"), (14341, "192.10.1.5"),
       (14345, "192.10.1.6"), (24341, "192.10.1.7")]

CASES = [
    # events inside one window: no callback
    case("test02NoMsg", 57, JMX, "query", "jmxMetric", [[I(15), L(T0 + i * 1000)] for i in range(5)],
         expected_count=0),
    # the trigger event must not join the batch it flushes
    case("test05EdgeCase", 100, JMX, "query", "jmxMetric",
         [[I(15), L(i * 10)] for i in range(3)] + [[I(85), L(10000 + i * 10)] for i in range(3)] +
         [[I(10000), L(100000)]],
         expected_count=2, expected_chunks=2, expected_chunk_sizes={"1": 2},
         expected_rows=[{"n": 1, "data": [D(15.0), L(3)]}, {"n": 2, "data": [D(85.0), L(3)]}]),
    # four rounds of three events 10 s apart and a fifth to flush the fourth.
    # The reference's selector also has max() / min() columns; this library
    # has neither aggregator, they are left out (the asserted count of output
    # events does not depend on them).
    case("test01DownSampling", 144,
         "define stream jmxMetric(cpu int, memory int, bytesIn long, bytesOut long, timestamp long);"
         "@info(name = 'downSample') from jmxMetric#window.externalTimeBatch(timestamp, 10 sec) "
         "select avg(cpu) as avgCpu,  '|' as s,  avg(memory) as avgMem,  '|' as s1,  avg(bytesIn) as avgBytesIn, "
         " '|' as s2,  avg(bytesOut) as avgBytesOut,  '|' as s3,  timestamp as timeWindowEnds,  '|' as s4, "
         " count() as metric_count  INSERT INTO tmp;",
         "downSample", "jmxMetric",
         [[I(15 + 10 * i * ite), I(1500 + 10 * i * ite), L(1000), L(2000), L(T0 + ite * 10000 + i * 50)]
          for ite in range(5) for i in range(3)],
         expected_count=4),
    case("test1", 226,
         "define stream inputStream(currentTime long,value int);  @info(name='query') "
         "from inputStream#window.externalTimeBatch(currentTime,5 sec) select value insert into outputStream; ",
         "query", "inputStream",
         [[L(t), I(v + 1)] for v, t in enumerate([10000, 11000, 12000, 13000, 14000, 15000, 16500, 17000, 18000,
                                                  19000, 20000, 20500, 22000, 25000])],
         expected_chunks=3,   # the first events of the three callbacks: 1, 6, 11
         expected_rows=[{"n": 1, "data": [I(1)]}, {"n": 6, "data": [I(6)]}, {"n": 11, "data": [I(11)]}]),
    # startTime 1200: the first window ends at 11200
    case("test2", 288,
         "define stream inputStream(currentTime long,value int);  @info(name='query') "
         "from inputStream#window.externalTimeBatch(currentTime,5 sec,1200) select value insert into outputStream; ",
         "query", "inputStream", [[L(i + 10000), I(i // 100)] for i in range(0, 10000, 100)],
         expected_rows=[{"n": 1, "data": [I(0)]}, {"n": 12, "data": [I(11)]}, {"n": 13, "data": [I(12)]}]),
    case("externalTimeBatchWindowTest2", 443, login("timestamp, 1 sec"), "query1", "LoginEvents", login_events(*SIX),
         expected_count=2, expected_remove_count=0),
    # the third event is exactly one window after the first: it flushes
    case("externalTimeBatchWindowTest3", 493, login("timestamp, 1 sec"), "query1", "LoginEvents",
         login_events(*(SIX[:2] + [(5341, "192.10.1.4")] + SIX[3:])), expected_count=3, expected_remove_count=0),
    # startTime 0, late events inside a batch
    case("externalTimeBatchWindowTest11", 953, login("timestamp, 1 sec, 0", ""), "query1", "LoginEvents",
         login_events((4341, "192.10.1.3"), (4599, "192.10.1.4"), (4600, "192.10.1.5"), (4607, "192.10.1.6"),
                      (5599, "192.10.1.4"), (5600, "192.10.1.5"), (5607, "192.10.1.6"), (5606, "192.10.1.7"),
                      (5605, "192.10.1.8"), (5606, "192.10.1.91"), (5605, "192.10.1.92"), (6606, "192.10.1.9"),
                      (6690, "192.10.1.10")),
         expected_count=2, expected_remove_count=0,
         expected_nth=[{"n": 1, "col": 2, "value": L(4)}, {"n": 2, "col": 2, "value": L(7)}]),
    # startTime read from the first event's attribute
    case("externalTimeBatchWindowTest14", 1113, login("timestamp, 1 sec, timestamp"), "query1", "LoginEvents",
         login_events(*SIX), expected_count=2, expected_remove_count=0),
    failure("externalTimeBatchWindowTest18", 1333, login("timestamp, 1 sec, 0, 100, 100")),
    failure("externalTimeBatchWindowTest19", 1392, login("timestamp")),
    failure("externalTimeBatchWindowTest20", 1442, login("timestamp, 1 sec, timestamp, 10.5")),
    failure("externalTimeBatchWindowTest21", 1485, login("timestamp, 1 sec, 1.0, 100, true")),
    failure("test22", 1534,
            "define stream inputStream(currentTime int,value int);  @info(name='query') "
            "from inputStream#window.externalTimeBatch(currentTime,5 sec) select value insert into outputStream; "),
    failure("test23", 1593,
            "define stream inputStream(currentTime int,value int);  @info(name='query') "
            "from inputStream#window.externalTimeBatch('currentTime',5 sec) select value "
            "insert into outputStream; "),
    failure("externalTimeBatchWindowTest25", 1696, login("timestamp, '1 sec', 123L, 100")),
    failure("externalTimeBatchWindowTest26", 1739, login("timestamp, 1 sec, 1/2, 100")),
]

if __name__ == "__main__":
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "ExternalTimeBatchWindowTestCase.json")
    with open(out, "w") as fp:
        json.dump(CASES, fp, indent=1)
        fp.write("\n")
    print("%d cases -> %s" % (len(CASES), out))
