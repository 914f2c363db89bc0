"""The environment switches, host side (no GPU).

a. The Evaluator's parse of MACR_EVAL_GRAPH, _SEEDS, _OPTIMISTIC, _FOLD, _FOLD_PREP and _FILTER: an evaluator built on the CPU
   (as tests/golden/make_golden_eval_policy.py builds its own) has the attribute values INTEGRATION.md documents.
b. The inventory: every MACR_* name the native sources read with getenv (directly, or through a helper that is handed the
   name) and the host layer reads from os.environ has a row in the table of INTEGRATION.md B.4 and occurs in at least one file
   under tests/ -- a switch no test names is an arm no test runs (tests/test_gpu_eval_switches.py and
   tests/test_gpu_switch_children.py run the arms themselves).
"""
import glob
import os
import re

import pytest

from macr_amd import _lib
from macr_amd.evaluator import Evaluator

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EVAL_VARS = ("MACR_EVAL_GRAPH", "MACR_EVAL_SEEDS", "MACR_EVAL_OPTIMISTIC", "MACR_EVAL_FOLD", "MACR_EVAL_FOLD_PREP", "MACR_EVAL_FILTER")


# ----------------------------------------------------------------------------- a. the evaluator's parse
def evaluator_under(monkeypatch, **env):
    for k in EVAL_VARS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    return Evaluator([[0]] * 3, [[1]] * 3, 4, "cpu")


def test_evaluator_defaults_without_any_variable(monkeypatch):
    ev = evaluator_under(monkeypatch)
    assert (ev.use_graph, ev.use_seeds, ev.optimistic) == (True, True, True)
    assert (ev.fold_prologue, ev.fold_metrics, ev.fold_prep) == (True, False, True)
    assert ev.filter == "f16" and ev.filter_now == "f16"


@pytest.mark.parametrize("var,attr", [("MACR_EVAL_GRAPH", "use_graph"), ("MACR_EVAL_SEEDS", "use_seeds"),
                                      ("MACR_EVAL_OPTIMISTIC", "optimistic"), ("MACR_EVAL_FOLD_PREP", "fold_prep")])
def test_on_off_switches_are_off_at_0_only(monkeypatch, var, attr):
    others = [a for a in ("use_graph", "use_seeds", "optimistic", "fold_prep") if a != attr]
    for value, want in (("0", False), ("1", True), ("", True)):
        ev = evaluator_under(monkeypatch, **{var: value})
        assert getattr(ev, attr) is want, (var, value)
        assert all(getattr(ev, a) is True for a in others), (var, value)          # one variable, one attribute
        assert (ev.fold_prologue, ev.fold_metrics, ev.filter) == (True, False, "f16")


@pytest.mark.parametrize("value,want", [("p", (True, False)), ("m", (False, True)), ("1", (True, True)), ("0", (False, False)),
                                        ("P", (True, False)), ("M", (False, True)), (" m ", (False, True)), ("\tp\n", (True, False)),
                                        (" 1", (True, True)), ("0 ", (False, False))])
def test_fold_values(monkeypatch, value, want):
    ev = evaluator_under(monkeypatch, MACR_EVAL_FOLD=value)
    assert (ev.fold_prologue, ev.fold_metrics) == want
    assert ev.fold_prep is True and ev.optimistic is True                          # (_FOLD does not reach _FOLD_PREP)


@pytest.mark.parametrize("value,want", [("f32", "f32"), ("bf16", "bf16"), ("f16", "f16"), ("F32", "f32"), (" BF16 ", "bf16")])
def test_filter_values(monkeypatch, value, want):
    ev = evaluator_under(monkeypatch, MACR_EVAL_FILTER=value)
    assert ev.filter == want and ev.filter_now == want


@pytest.mark.parametrize("value", ["f61", "fp16", "", "1"])
def test_filter_typo_is_refused_by_name(monkeypatch, value):
    with pytest.raises(_lib.MacrError) as e:
        evaluator_under(monkeypatch, MACR_EVAL_FILTER=value)
    assert repr(value.strip().lower()) in str(e.value) and "'f16'" in str(e.value)


# ----------------------------------------------------------------------------- b. the inventory
_NAME = r"MACR_[A-Z0-9_]+"
_PART_B = "# " + "-" * 77 + " b. the inventory"
# name -> why it has no table row or no test reference.  (Nothing: every switch is documented and named by a test.)
EXEMPT = {}


def names_read_by_the_code():
    found = {}
    for path in sorted(glob.glob(os.path.join(REPO, "macr_amd", "csrc", "*.hip")) + glob.glob(os.path.join(REPO, "macr_amd", "csrc", "*.hpp"))):
        with open(path) as f:
            # getenv("MACR_X"), and a name handed to a helper that calls getenv (read_plan_knobs' at_least("MACR_SPMM_T", ..)):
            # a string literal that is nothing but such a name
            for name in re.findall(r'"(%s)"' % _NAME, f.read()):
                found.setdefault(name, os.path.relpath(path, REPO))
    for path in sorted(glob.glob(os.path.join(REPO, "macr_amd", "*.py"))):
        with open(path) as f:
            for name in re.findall(r'os\.environ(?:\.get)?\s*[\[(]\s*["\'](%s)["\']' % _NAME, f.read()):
                found.setdefault(name, os.path.relpath(path, REPO))
    return found


def names_with_a_table_row():
    """the names in the first cell of every row of INTEGRATION.md's `| variable | effect |` table"""
    with open(os.path.join(REPO, "INTEGRATION.md")) as f:
        lines = f.read().splitlines()
    start = lines.index("| variable | effect |")
    rows = set()
    for line in lines[start + 2:]:
        if not line.startswith("|"):
            break
        cell = re.split(r"(?<!\\)\|", line)[1]
        rows.update(re.findall(_NAME, cell))
    return rows


def names_in_tests():
    me = os.path.abspath(__file__)
    text = []
    for root, _, files in os.walk(os.path.join(REPO, "tests")):
        for name in files:
            path = os.path.join(root, name)
            if name.endswith((".py", ".json", ".txt", ".md")):
                with open(path, errors="replace") as f:
                    # (of this file, part a only: the lists of part b name switches without running anything)
                    text.append(f.read().split(_PART_B)[0] if os.path.abspath(path) == me else f.read())
    return set(re.findall(_NAME, "\n".join(text)))


def test_the_scan_finds_the_switches_it_is_for():
    found = names_read_by_the_code()
    for name in ("MACR_STAGE_LISTED", "MACR_STAGING", "MACR_EVAL_F32_SAMPLE", "MACR_LGCN_DENSE", "MACR_SORT_TILE", "MACR_SPMM_T",   # native
                 "MACR_EVAL_FOLD", "MACR_SWEEP_ONE_BY_ONE", "MACR_LAZY_ADAM_MF", "MACR_HIP_LIB"):                        # host
        assert name in found, name
    assert len(found) >= 35, sorted(found)


def test_every_switch_has_a_table_row_and_a_test_that_names_it():
    found, rows, tested = names_read_by_the_code(), names_with_a_table_row(), names_in_tests()
    assert not set(EXEMPT) - set(found), "exemptions of names nothing reads: %s" % sorted(set(EXEMPT) - set(found))
    no_row = sorted("%s (%s)" % (n, found[n]) for n in found if n not in rows and n not in EXEMPT)
    no_test = sorted("%s (%s)" % (n, found[n]) for n in found if n not in tested and n not in EXEMPT)
    assert not no_row, "read by the code, no row in INTEGRATION.md B.4: %s" % no_row
    assert not no_test, "read by the code, named by no file under tests/: %s" % no_test
