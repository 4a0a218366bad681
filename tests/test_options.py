"""The tuning options of the native library are read in ONE unit (csrc/options.h + options.cpp) and pconv_option
shows what it read (include/pconv_hip.h).  No GPU and no kernel launch: with a NULL engine the query reads the
environment like a create or a call made now would."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pseudocylindrical_convolution_amd", "csrc")
AUTO = -2 ** 31   # PCONV_OPTION_AUTO: unset, the library decides

# the documented defaults ("What runs by default"; codes: include/pconv_hip.h)
DEFAULTS = {
    "PCONV_EE_BLOCK": 256, "PCONV_EE_PPW": 0, "PCONV_EE_JOINT": 2, "PCONV_EE_CONTIG": 1, "PCONV_EE_XCD": 0,
    "PCONV_EE_FUSE_PPW": 4, "PCONV_EE_MFMA_WSRC": 0, "PCONV_EE_MFMA_WAVES": 4, "PCONV_EE_MFMA_NT": 1,
    "PCONV_ENGINE_GROUPS": AUTO, "PCONV_ENGINE_WORKERS": AUTO, "PCONV_ENGINE_CHAIN": AUTO,
    "PCONV_ENGINE_BLOCKING_SYNC": AUTO, "PCONV_ENGINE_SPIN_US": AUTO, "PCONV_ENGINE_ROWS": 0,
    "PCONV_ENGINE_STEPWISE_ENCODER": 0, "PCONV_ENGINE_CLEAR_EVERY_CALL": 0, "PCONV_ENGINE_ALLOC_FILL": -1,
    "PCONV_ENGINE_ENCODE_RANGES": 4,
    "PCONV_ENGINE_ENCODE_INTERLEAVE": 1, "PCONV_ENGINE_RATE_STREAMS": 0, "PCONV_ENGINE_TIMING": 0,
    "PCONV_EE_BULK": 0, "PCONV_EE_BULK0": 0, "PCONV_EE_MFMA_FORM": 0, "PCONV_EE_FUSE_TABLES": 0,
    "PCONV_ENGINE_CU_MASK_FIRST": 0, "PCONV_ENGINE_CU_MASK_COUNT": 0,
    "PCONV_CONV1X1": 0, "PCONV_CONV1X1_STAGGER": -1, "PCONV_CONV1X1_WAYOUT": 0, "PCONV_CONV_SMALL": 1,
    "PCONV_CONV_XCD": 0, "PCONV_RESAMPLE_ROWS": 2,
}
NOT_QUERIED = {"PCONV_ENGINE_CU_MASK", "PCONV_CGROUP_CPU_MAX"}   # first:count (reported as _FIRST / _COUNT); a path


def unit_names():
    """every PCONV_ variable the options unit names"""
    text = "".join(open(os.path.join(CSRC, f)).read() for f in ("options.h", "options.cpp"))
    return set(re.findall(r'"(PCONV_[A-Z0-9_]+)"', text))


@pytest.fixture()
def option(monkeypatch):
    from pseudocylindrical_convolution_amd import _native
    for name in unit_names():
        monkeypatch.delenv(name, raising=False)
    return _native.option


def test_every_option_reports_its_documented_default(option):
    assert unit_names() - NOT_QUERIED == set(DEFAULTS)       # the table above is the unit's list, no more, no less
    for name, value in DEFAULTS.items():
        assert option(name) == value, name


def test_a_null_engine_follows_the_environment(option, monkeypatch):
    monkeypatch.setenv("PCONV_EE_FUSE_PPW", "2")                                    # a number
    assert option("PCONV_EE_FUSE_PPW") == 2
    monkeypatch.setenv("PCONV_ENGINE_ROWS", "int32")                                # a first letter
    assert option("PCONV_ENGINE_ROWS") == 1
    monkeypatch.setenv("PCONV_ENGINE_ROWS", "packed")
    assert option("PCONV_ENGINE_ROWS") == 0
    monkeypatch.setenv("PCONV_ENGINE_CHAIN", "host")
    assert option("PCONV_ENGINE_CHAIN") == 0
    monkeypatch.setenv("PCONV_ENGINE_CHAIN", "queued")
    assert option("PCONV_ENGINE_CHAIN") == 1
    monkeypatch.setenv("PCONV_CONV1X1_WAYOUT", "batch")
    assert option("PCONV_CONV1X1_WAYOUT") == 2
    monkeypatch.setenv("PCONV_ENGINE_CU_MASK", "8:64")
    assert (option("PCONV_ENGINE_CU_MASK_FIRST"), option("PCONV_ENGINE_CU_MASK_COUNT")) == (8, 64)
    monkeypatch.setenv("PCONV_ENGINE_TIMING", "")                                   # counts by being set
    assert option("PCONV_ENGINE_TIMING") == 1
    from pseudocylindrical_convolution_amd import _native
    monkeypatch.setenv("PCONV_ENGINE_SPIN_US", "137")                               # the query and the stateless
    assert option("PCONV_ENGINE_SPIN_US") == 137                                    # entry point read the same value
    assert _native.hip_lib().pconv_ee_spin_us(8) == 137
    monkeypatch.delenv("PCONV_ENGINE_SPIN_US")
    assert option("PCONV_ENGINE_SPIN_US") == AUTO
    assert _native.hip_lib().pconv_ee_spin_us(8) in (60, 2000)


def test_an_unknown_name_is_refused(option):
    from pseudocylindrical_convolution_amd import _native
    with pytest.raises(_native.PconvError, match="unknown name PCONV_NO_SUCH_OPTION"):
        option("PCONV_NO_SUCH_OPTION")
    with pytest.raises(_native.PconvError):
        option("PCONV_ENGINE_CU_MASK")                       # reported under its two names


def test_only_the_options_unit_reads_the_environment():
    for f in sorted(os.listdir(CSRC)):
        if f in ("options.h", "options.cpp"):
            continue
        text = open(os.path.join(CSRC, f)).read()
        assert 'getenv("PCONV_' not in text, "%s reads a PCONV_ variable itself" % f
        for name in re.findall(r"getenv\(\s*\"?(\w+)", text):
            assert name == "LOCAL_WORLD_SIZE", "%s: getenv(%s)" % (f, name)


def xmacro_names():
    """the variable of every X(...) row of options.h, in the file's order"""
    return re.findall(r'\bX\("(PCONV_[A-Z0-9_]+)",', open(os.path.join(CSRC, "options.h")).read())


def test_every_option_has_a_gpu_test():
    """tests/option_cases.py names, for every option row of options.h, a GPU test that launches the code the option
    selects: the test exists in the file named (read with ast: nothing of it is imported), its source names the option,
    and the values that once had no launch at all stay listed"""
    import ast
    import option_cases
    names = xmacro_names()
    assert len(names) == len(set(names)) >= 31
    assert set(option_cases.OPTIONS) == set(names), "tests/option_cases.py and options.h list different options: %s" % sorted(
        set(option_cases.OPTIONS) ^ set(names))
    assert set(names) == set(DEFAULTS) - {"PCONV_ENGINE_CU_MASK_FIRST", "PCONV_ENGINE_CU_MASK_COUNT"}   # every row was found
    sources = {}
    for name in names:
        row = option_cases.OPTIONS[name]
        assert row.values and all(isinstance(v, str) and v for v in row.values), name
        assert row.file.startswith("test_gpu_"), (name, row.file)
        if row.file not in sources:
            text = open(os.path.join(ROOT, "tests", row.file)).read()
            tree = ast.parse(text)
            marked = any(isinstance(n, ast.Assign) and any(getattr(t, "id", None) == "pytestmark" for t in n.targets) and
                         "pytest.mark.gpu" in ast.get_source_segment(text, n) for n in tree.body)
            sources[row.file] = ({n.name: ast.get_source_segment(text, n) for n in tree.body if isinstance(n, ast.FunctionDef)},
                                 marked)
        tests, marked = sources[row.file]
        assert marked, "%s is not a GPU test file" % row.file
        assert row.test in tests, "%s: no test %s in tests/%s" % (name, row.test, row.file)
        assert re.search(r"\b%s\b" % name, tests[row.test]), "%s::%s does not name %s" % (row.file, row.test, name)
    for name, values in option_cases.MUST_RUN.items():
        assert set(values) <= set(option_cases.OPTIONS[name].values), (name, values, option_cases.OPTIONS[name].values)
    assert len(option_cases.MUST_RUN) == 10


def test_every_option_has_a_row_in_the_default_table():
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    section = design.split("## What runs by default", 1)[1].split("\n## ", 1)[0]
    rows = [line for line in section.splitlines() if line.startswith("| `PCONV_")]
    named = set(re.findall(r"`(PCONV_[A-Z0-9_]+)`", " ".join(r.split("|")[1] for r in rows)))
    missing = {n for n in unit_names() if n not in named and not n.startswith("PCONV_ENGINE_CU_MASK_")}
    assert not missing, "no row in DESIGN.md's table: %s" % sorted(missing)
    for row in rows:
        assert len(row.split("|")) == 7, row                # option, default, other values, lifetime, decided by
