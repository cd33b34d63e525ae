"""What the tracking step keeps off the voxels' chain: tools/step_loop_stats.py --chain on lean units a and b, without a GPU.

The step is latency bound, and its longest link is the wait for the four grid gathers.  The exponential of the step (an LDS table read
with a wait of its own and a dozen dependent fp64 operations) and the logarithm read no voxel, so they stand between the issue of the
gathers and their wait (VolpathMachine::step_fast), where a wave has nothing else to do; the parent of the change that brought this
test started the exponential only when the voxels had arrived (profiles/step_chain_trips_parent.txt / step_chain_trips.txt).

For the common path of each in-place repeat loop of wg_block (B_MED: main path, B_MEDW: walks) the tool lists the instructions that are
a ds_read* or carry _f64 in the mnemonic and lie on some path from the gathers' s_waitcnt vmcnt(0) to the loop's back edge: none may
be left.  Each common path holds one ds_read_b128 and one ds_read_b64 -- one logarithm and one exponential per round.

One device-only compile of each unit to assembly (about 30 s), shared by the unit's cases."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def tool():
    spec = importlib.util.spec_from_file_location("step_loop_stats", os.path.join(ROOT, "tools", "step_loop_stats.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def chains(tool, tmp_path_factory):
    done = {}
    def get(unit):
        if unit not in done:
            asm = str(tmp_path_factory.mktemp("step_chain") / (unit + ".s"))
            tool.compile_asm(unit, asm)
            done[unit] = tool.chain(asm)
            print(unit)
            print(tool.render_chain(done[unit]))
        return done[unit]
    return get


@pytest.mark.parametrize("loop", ["B_MED", "B_MEDW"])
@pytest.mark.parametrize("unit", ["kernels_lean_a.hip", "kernels_lean_b.hip"])
def test_no_table_read_and_no_fp64_chain_waits_for_a_voxel(chains, unit, loop):
    r = chains(unit)[loop]
    assert r["behind"] == [], "%s of %s: behind the wait for the grid gathers stand %s" % (loop, unit, r["behind"])
    assert r["reads"] == {"ds_read_b128": 1, "ds_read_b64": 1}, r["reads"]      # one logarithm and one exponential per round
