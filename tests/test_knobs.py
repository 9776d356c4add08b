"""The SHD_* environment switches (siddhi_amd/csrc/knobs.h): the three parsers,
and the registry against the sources, the tests and scripts that set the
variables, and the table in DESIGN.md.  CPU only: knobs.h is compiled into a
stand-alone program with the host C++ compiler."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "siddhi_amd", "csrc")


def registry():
    """{environment name: (kind, when)} from the X-macro list of knobs.h."""
    text = open(os.path.join(CSRC, "knobs.h")).read()
    entries = re.findall(r'^\s*X\((\w+),\s*"(SHD_[A-Z0-9_]+)",\s*(\w+),\s*(\w+),\s*"[^"]+"\)', text, re.M)
    assert len(entries) == len(re.findall(r"^\s*X\(", text, re.M)), "an entry of SHD_KNOBS did not parse"
    assert len({e[0] for e in entries}) == len(entries) and len({e[1] for e in entries}) == len(entries)
    for ident, name, kind, when in entries:
        assert name == "SHD_" + ident, (ident, name)
        assert kind in ("FLAG", "TRISTATE", "INT") and when in ("PROCESS", "LOAD", "PUSH"), name
    return {name: (kind, when) for _, name, kind, when in entries}


def design_rows():
    """[(name, kind, when, role)] of the table in DESIGN.md's "Environment switches"."""
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    m = re.search(r"^## [^\n]*Environment switches\n(.*?)(?=^## |\Z)", text, re.M | re.S)
    assert m, 'DESIGN.md has no "Environment switches" section'
    return re.findall(r"^\| `(SHD_[A-Z0-9_]+)` \| (\w+) \| (\w+) \| ([^|]+?) \|", m.group(1), re.M)


# ---------------------------------------------------------------- the parsers
PROGRAM = r"""
#include <cstdio>
#include "knobs.h"
using namespace shd;
int main() {
  for (int i = 0; i < kNumKnobs; i++) {
    const Knob k = (Knob)i;
    switch (kKnobs[i].kind) {
      case KnobKind::FLAG: std::printf("%s FLAG %d\n", kKnobs[i].name, knob_on(k) ? 1 : 0); break;
      case KnobKind::TRISTATE: std::printf("%s TRISTATE %d\n", kKnobs[i].name, knob_force(k)); break;
      case KnobKind::INT: {
        int v = 12345;
        if (knob_int(k, v)) std::printf("%s INT %d\n", kKnobs[i].name, v);
        else std::printf("%s INT unset\n", kKnobs[i].name);
        break;
      }
    }
  }
  return 0;
}
"""


@pytest.fixture(scope="module")
def parse(tmp_path_factory):
    """parse(env) -> {name: (kind, value)} as the compiled accessors see `env`."""
    d = tmp_path_factory.mktemp("knobs")
    src = d / "knobs_main.cpp"
    src.write_text(PROGRAM)
    exe = d / "knobs_main"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-I", CSRC, str(src), "-o", str(exe)])
    base = {k: v for k, v in os.environ.items() if not k.startswith("SHD_")}

    def run(env):
        out = subprocess.check_output([str(exe)], env=dict(base, **env)).decode()
        return {name: (kind, value) for name, kind, value in (line.split() for line in out.splitlines())}
    return run


def names_of(kind):
    return [n for n, (k, _) in registry().items() if k == kind]


def expect(parse, env, kind, value):
    """Every knob of `kind` parses to `value` under `env`; every other knob
    reads as unset."""
    got = parse(env)
    reg = registry()
    assert list(got) == list(reg), "the program lists the registry in order"
    unset = {"FLAG": "0", "TRISTATE": "-1", "INT": "unset"}
    for name, (k, _) in reg.items():
        assert got[name] == (k, value if k == kind else unset[k]), (name, env.get(name))


def test_nothing_set(parse):
    expect(parse, {}, None, None)


@pytest.mark.parametrize("text,value", [("1", "1"), ("0", "0"), ("", "0"), ("on", "1"), ("00", "0")])
def test_flag(parse, text, value):
    expect(parse, {n: text for n in names_of("FLAG")}, "FLAG", value)


@pytest.mark.parametrize("text,value", [("0", "0"), ("1", "1"), ("", "-1"), ("on", "1")])
def test_tristate(parse, text, value):
    assert sorted(names_of("TRISTATE")) == ["SHD_FUSED_SORT", "SHD_LOCKSTEP", "SHD_NFA_WINDOW"]
    expect(parse, {n: text for n in names_of("TRISTATE")}, "TRISTATE", value)


@pytest.mark.parametrize("text,value", [("8", "8"), ("0", "0"), ("-3", "-3"), ("x", "0"), ("", "unset")])
def test_int(parse, text, value):
    assert sorted(names_of("INT")) == ["SHD_HASH_BITS", "SHD_NFA_CHUNK", "SHD_NFA_EVENTS", "SHD_NFA_LIST",
                                       "SHD_NFA_PARTIALS", "SHD_NFA_RECORDS", "SHD_NFA_TIMERS", "SHD_RESUME_MODE"]
    expect(parse, {n: text for n in names_of("INT")}, "INT", value)


def test_wrong_kind_is_caught(tmp_path):
    """Asking a knob through another kind's accessor trips the assert."""
    src = tmp_path / "wrong.cpp"
    src.write_text('#include "knobs.h"\nint main() { return shd::knob_on(shd::Knob::HASH_BITS) ? 1 : 0; }\n')
    exe = tmp_path / "wrong"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-I", CSRC, str(src), "-o", str(exe)])
    r = subprocess.run([str(exe)], stderr=subprocess.PIPE)
    assert r.returncode not in (0, 1) and b"info.kind == kind" in r.stderr


# --------------------------------------------------------------- the registry
def files_under(top, skip_dirs=("build", "__pycache__", "golden")):
    for d, dirs, files in os.walk(top):
        dirs[:] = [x for x in dirs if x not in skip_dirs]
        for f in sorted(files):
            if not f.endswith((".so", ".pyc", ".o")):
                yield os.path.join(d, f)


def test_library_reads_the_environment_through_the_registry_only():
    reg = registry()
    seen = set()
    for path in files_under(CSRC):
        text = open(path, errors="replace").read()
        rel = os.path.relpath(path, ROOT)
        if os.path.basename(path) != "knobs.h":
            assert "getenv" not in text, "%s calls getenv: add a knob to knobs.h instead" % rel
        for name in re.findall(r'"(SHD_[A-Z0-9_]+)"', text):
            assert name in reg, "%s: %s is not in knobs.h" % (rel, name)
            seen.add(name)
    assert seen == set(reg)


# the forms in which a test or a script names an environment variable
ENV_FORMS = [r"""(?:setenv|delenv)\(\s*["'](SHD_[A-Z0-9_]+)["']""",      # monkeypatch.setenv / delenv
             r"""\bexport\s+(SHD_[A-Z0-9_]+)""",                         # shell export
             r"""["'](SHD_[A-Z0-9_]+)["']\s*:""",                        # key of an environment dict
             r"""environ(?:\.get\(|\.pop\(|\.setdefault\(|\[)\s*["'](SHD_[A-Z0-9_]+)["']"""]   # os.environ


def test_every_variable_the_tests_and_scripts_set_exists():
    reg = registry()
    python_rows = {n for n, kind, _, _ in design_rows() if kind == "python"}
    found = {}
    for top in ("tests", "scripts"):
        for path in files_under(os.path.join(ROOT, top)):
            text = open(path, errors="replace").read()
            for form in ENV_FORMS:
                for name in re.findall(form, text):
                    found.setdefault(name, os.path.relpath(path, ROOT))
    # the forms do find what is there: a setenv, a dict key, a shell export
    assert {"SHD_FUSED_SORT", "SHD_NFA_PARTIALS", "SHD_LIB"} <= set(found)
    for name, where in sorted(found.items()):
        assert name in reg or name in python_rows, "%s sets %s, which nothing reads" % (where, name)


def test_design_table_matches_the_registry():
    rows = design_rows()
    assert len({n for n, _, _, _ in rows}) == len(rows), "a knob is listed twice"
    table = {n: (kind, when) for n, kind, when, _ in rows if kind != "python"}
    assert table == registry()
    assert {n for n, kind, _, _ in rows if kind == "python"} == {"SHD_LIB", "SHD_ROUTE_TORCH", "SHD_ROUTE_SYNC"}
    # the library keeps no A/B leftovers: a concluded experiment's losing side is deleted
    roles = {role for _, _, _, role in rows}
    assert roles == {"test hook", "override", "diagnostic", "A/B leftover"}, roles
    assert {n for n, kind, _, role in rows if role == "A/B leftover" and kind != "python"} == set()
    assert {n for n, _, _, role in rows if role == "A/B leftover"} == {"SHD_ROUTE_TORCH", "SHD_ROUTE_SYNC"}
