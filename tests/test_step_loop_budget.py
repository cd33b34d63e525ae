"""Static budget of the tracking step: tools/step_loop_stats.py on lean unit a (the metric scene's kernel), without a GPU.

The tool compiles kernels_lean_a.hip to assembly with the product flags and finds the two in-place repeat loops of wg_block (B_MED:
main path, B_MEDW: NEE / direct-light walks) through the line table.  Ceilings on the instructions and the divergent regions
(*saveexec*) of each loop's common path -- the loop without the blocks behind its one branch to the rare path -- and of the whole loop,
rare path included.  Measured on the tree this test came with (parent commit in brackets, whose loops have no rare path):

                      common path                      whole loop
    B_MED    instructions 627 (891)   regions 7 (51)    instructions 1891   regions 66
    B_MEDW   instructions 507 (774)   regions 7 (46)    instructions 1634   regions 61

The ceilings are those figures plus 5 %, rounded down: room for a compiler patch release, not for a regression."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEASURED = {"B_MED": {"common": (627, 7), "whole": (1891, 66)}, "B_MEDW": {"common": (507, 7), "whole": (1634, 61)}}
PARENT_REGIONS = {"B_MED": 51, "B_MEDW": 46}


@pytest.fixture(scope="module")
def loops():
    spec = importlib.util.spec_from_file_location("step_loop_stats", os.path.join(ROOT, "tools", "step_loop_stats.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool.measure("kernels_lean_a.hip")


@pytest.mark.parametrize("loop", ["B_MED", "B_MEDW"])
def test_step_loop_stays_within_its_budget(loops, loop):
    whole, _, common, _ = loops[loop]
    for name, s in (("common", common), ("whole", whole)):
        got = (s["instructions"], s["divergent regions (*saveexec*)"])
        print(loop, name, "instructions %d, divergent regions %d" % got)
        insts, regions = MEASURED[loop][name]
        assert got[0] <= insts * 105 // 100 and got[1] <= regions * 105 // 100, (loop, name, got)
    # the design goal: the common path holds at most half the divergent regions of the parent's loop, and is shorter than it
    assert 2 * common["divergent regions (*saveexec*)"] <= PARENT_REGIONS[loop]
    assert common["scratch_"] == 0
