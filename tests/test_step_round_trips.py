"""Memory round trips of the tracking step: tools/step_loop_stats.py --trips on lean unit a (the metric scene's kernel), without a GPU.

The step is bound by the length of its dependent chains, and a chain's longest links are its waits for memory.  The tool lists, for the
common path of each in-place repeat loop of wg_block (B_MED: main path, B_MEDW: walks), the memory instructions and the s_waitcnt
between them in control-flow order, and checks three rules on the control-flow graph of the assembly:

  (a) the gathers of grid_fetch_pair go out together: no path leads from one global_load_dwordx4 to another through an s_waitcnt that
      names vmcnt (short of a back edge).  The parent of the change that brought this test issued the gathers of the second pair of
      rows only after the first pair had arrived (profiles/gather_trips_ab.txt holds both listings).
  (b) the same for the medium record's s_load and lgkmcnt: the step makes a lane whose medium has no invariant reciprocal rare by value
      instead of branching on the record's first 32 bytes, so the whole record arrives in one scalar trip.
  (c) the logarithm's table read (ds_read_b128) before the record's first s_load: reported, NOT asserted -- that form was measured and
      left out.

One device-only compile of the unit to assembly (about 30 s), shared by both cases."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def trips(tmp_path_factory):
    spec = importlib.util.spec_from_file_location("step_loop_stats", os.path.join(ROOT, "tools", "step_loop_stats.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    asm = str(tmp_path_factory.mktemp("step_trips") / "unit.s")
    tool.compile_asm("kernels_lean_a.hip", asm)
    res = tool.trips(asm)
    print(tool.render_trips(res))
    return res


@pytest.mark.parametrize("loop", ["B_MED", "B_MEDW"])
def test_gathers_and_medium_record_go_out_in_one_round_trip_each(trips, loop):
    r = trips[loop]
    gathers = [l for l in r["listing"] if " global_load_dwordx4 " in l]
    assert len(gathers) == 4, gathers                          # the common path holds one lookup: two z-levels x two y-rows
    assert [l for l in r["listing"] if "<- medium record" in l], "no scalar load of the medium record found in %s" % loop
    assert r["a"] == [], "a gather of %s is issued behind the wait for another one: %s" % (loop, r["a"])
    assert r["b"] == [], "a load of the medium record in %s is issued behind the wait for another one: %s" % (loop, r["b"])
    print(loop, "(c) logarithm's table read ahead of the record:", not r["c"])
