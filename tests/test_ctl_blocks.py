"""The per-push readback blocks (the *Totals structs of siddhi_amd/csrc): no
source addresses a field of a device or pinned buffer by a literal index or a
literal byte offset any more.  The layouts themselves are pinned by the
static_asserts next to each struct, which the build checks.  CPU only."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "siddhi_amd", "csrc")

# buf.as<T>() + 3, / ; / )   and   buf.as<T>()[3]
LITERAL_INDEX = re.compile(r"\.as<[^>]+>\(\)\s*(\+\s*\d+\s*[,;)]|\[\d+\])")
# buf.as<char>() + 64
LITERAL_BYTES = re.compile(r"\.as<char>\(\)\s*\+\s*\d+")


def sources():
    for d, dirs, files in os.walk(CSRC):
        dirs[:] = [x for x in dirs if x != "build"]
        for f in sorted(files):
            if f.endswith((".hip", ".h", ".cpp")):
                yield os.path.join(d, f)


def test_the_patterns_find_the_forms_they_are_about():
    for text in ("d_tot.as<uint64_t>() + 2;", "f(d_tot.as<uint64_t>() + 9, d_scan)", "(d_tot.as<uint64_t>() + 5))",
                 "h_tot.as<uint32_t>()[14]", "hctr.as<uint32_t>()[0]"):
        assert LITERAL_INDEX.search(text), text
    for text in ("d_agg.as<char>() + 232)", "h_ctl.as<char>() + 128,"):
        assert LITERAL_BYTES.search(text), text
    # array strides are not field offsets
    for text in ("d_bcnt.as<uint32_t>() + 2 * ntile,", "d_now.as<int64_t>() + (ncalls - 1),",
                 "arg_host.as<char>() + off,", "*h_last.as<int64_t>()"):
        assert not LITERAL_INDEX.search(text) and not LITERAL_BYTES.search(text), text


def test_no_source_addresses_a_buffer_by_a_literal():
    paths = list(sources())
    assert len(paths) >= 18, "the walk found the library's sources"
    hits = []
    for path in paths:
        text = open(path, errors="replace").read()
        for pat in (LITERAL_INDEX, LITERAL_BYTES):
            for m in pat.finditer(text):
                hits.append("%s:%d: %s" % (os.path.relpath(path, ROOT), text.count("\n", 0, m.start()) + 1, m.group(0)))
    assert not hits, "name the field in the block's struct instead:\n" + "\n".join(hits)


def test_every_block_pins_its_device_layout():
    """Each readback struct comes with a static_assert on its offsets."""
    text = "".join(open(p, errors="replace").read() for p in sources())
    blocks = set(re.findall(r"ReadbackBlock<(\w+)", text))
    assert {"PatternTotals", "SingleTotals", "AbsentTotals", "WindowTotals", "GDictTotals"} <= blocks
    for name in blocks:
        assert re.search(r"static_assert\(offsetof\(%s, " % name, text), name
