"""The host arithmetic of mts_render (csrc/render_plan.cpp) on the CPU: spiral, shards and launches, film slots and the wavefront split,
the smoothing of measured tile costs, the cost-sorted schedule, the render switches, and the kernel table with the choice of a scene's
render kernel.  GPU films cannot see any of it by design (the
order of blocks and tiles changes no pixel), so it is pinned here against restatements in Python.

render_plan.cpp is compiled with g++ next to an extern "C" shim (tests/micro/render_plan_shim.cpp) and loaded by ctypes."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import tests.kernel_rows as kr
import tests.oracle_binding as ob

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "eradiate-kernel_amd", "csrc")
SWITCHES = ("MTSAMD_KERNEL", "MTSAMD_LEAN", "MTSAMD_LPT", "MTSAMD_LPT_DEBUG", "MTSAMD_PASS_SLOTS", "MTSAMD_WAVEFRONT_SPLIT", "MTSAMD_TEST_INJECT_LOST_PATH")
i64p, u32p, u64p, i32p = (np.ctypeslib.ndpointer(t, flags="C_CONTIGUOUS") for t in (np.int64, np.uint32, np.uint64, np.int32))


@pytest.fixture(scope="module")
def L(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("render_plan") / "librender_plan.so")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-Wall", "-shared", "-fPIC", "-I", CSRC,
                           os.path.join(ROOT, "tests", "micro", "render_plan_shim.cpp"), os.path.join(CSRC, "render_plan.cpp"), "-o", out])
    lib = C.CDLL(out)
    lib.rp_spiral.argtypes = [C.c_int] * 7 + [i32p]
    lib.rp_switches.argtypes = [i64p, C.c_char_p]
    lib.rp_plan.argtypes = [i32p] + [C.c_int32] * 5 + [C.c_int] * 3 + [C.c_int64, i64p, u32p, i64p, C.c_char_p]
    lib.rp_lpt_policy.argtypes = [C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_int64, C.c_int64, C.c_int, C.c_int, i64p, C.c_char_p]
    lib.rp_calibration_blocks.argtypes = [u32p, C.c_int64, u32p, i64p, C.c_char_p]
    lib.rp_smooth.argtypes = [u64p, u32p, C.c_int64, C.c_uint32, i32p, u64p, u32p, C.c_int, C.c_uint32, C.c_char_p]
    lib.rp_choose_kernel.argtypes = [i32p, C.c_int64, C.c_uint32, i32p, C.c_char_p]
    lib.rp_kernel_rows.argtypes = [i32p, i32p, i32p]
    lib.rp_schedule.argtypes = [u32p, C.c_int64, u64p, u32p, C.c_int64, u64p, C.c_int64, C.c_uint32, C.c_int, C.c_uint32, C.c_int64, u32p, i64p, C.c_char_p]
    return lib


@pytest.fixture
def env(monkeypatch):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    return monkeypatch


def call(fn, *args):
    err = C.create_string_buffer(512)
    if fn(*args, err) != 0:
        raise RuntimeError(err.value.decode())


def blocks_of(rows):
    """DBlock records (ox, oy, sx, sy, id, sample_base, film_off_lo, film_off_hi) as an (n, 8) uint32 array."""
    return np.ascontiguousarray(np.array(rows, dtype=np.int64).astype(np.uint32).reshape(-1, 8))


def plan(L, crop, spp, spp_per_pass=-1, block_size=32, wavefront=0, channels=5, shard=(0, 1), cus=256):
    cap = 1 << 16
    head, blocks, sizes = np.zeros(10, np.int64), np.zeros((cap, 8), np.uint32), np.zeros(cap, np.int64)
    call(L.rp_plan, np.array(crop, np.int32), spp, wavefront, spp_per_pass, block_size, channels, shard[0], shard[1], cus, cap, head, blocks, sizes)
    keys = ("block_size", "n_passes", "split", "launch_spp", "film_floats", "n_slots", "pass_slots", "samples", "n_chunks", "n")
    p = dict(zip(keys, (int(v) for v in head)))
    assert p["n"] <= cap
    p["blocks"], p["chunk_sizes"] = blocks[:p["n"]], sizes[:p["n_chunks"]]
    return p


def oracle_spiral(w, h, x, y, bs, passes):
    n = ((w + bs - 1) // bs) * ((h + bs - 1) // bs) * passes
    out = (C.c_int32 * (5 * n))()
    assert ob.lib().oracle_spiral(w, h, x, y, bs, passes, n, out) == n
    return np.array(out[:]).reshape(n, 5)


def morton_origin(t):
    m, x, y = 16 * t, 0, 0
    for bit in range(16):
        x |= ((m >> (2 * bit)) & 1) << bit
        y |= ((m >> (2 * bit + 1)) & 1) << bit
    return x, y


# ---------------------------------------------------------------- spiral, shards, launches
@pytest.mark.parametrize("w,h,x,y,bs,passes", [(318, 322, 0, 0, 32, 1), (20, 20, 0, 0, 32, 1), (41, 30, 7, 5, 8, 1),
                                               (97, 13, 3, 11, 16, 3), (64, 64, 0, 0, 16, 4)])
def test_spiral_equals_the_oracle(L, w, h, x, y, bs, passes):
    ref = oracle_spiral(w, h, x, y, bs, passes)
    out = np.zeros(5 * len(ref) + 5, np.int32)
    assert L.rp_spiral(w, h, x, y, bs, passes, len(ref) + 1, out) == len(ref)
    assert np.array_equal(out[:5 * len(ref)].reshape(-1, 5), ref)


@pytest.mark.parametrize("crop,spp,spp_per_pass,bs,shards", [((0, 0, 96, 64), 8, 4, 16, 4), ((7, 5, 41, 30), 12, 4, 8, 3),
                                                             ((0, 0, 2048, 2048), 8, 2, 512, 1), ((0, 0, 4096, 1024), 6, 2, 1024, 5)])
def test_shards_and_chunks_cover_every_pass_and_block_once(L, env, crop, spp, spp_per_pass, bs, shards):
    passes = spp // spp_per_pass
    ref = oracle_spiral(crop[2], crop[3], crop[0], crop[1], bs, passes)
    max_blocks = max(1, (8 << 20) // (bs * bs))
    seen, samples = [], 0
    for shard in range(shards):
        p = plan(L, crop, spp, spp_per_pass, bs, shard=(shard, shards))
        assert (p["block_size"], p["n_passes"], p["split"], p["launch_spp"]) == (bs, passes, 1, spp_per_pass)
        assert p["chunk_sizes"].sum() == p["n"] and p["chunk_sizes"].max() <= max_blocks
        assert (p["chunk_sizes"][:-1] == max_blocks).all()                  # the chunks cut the one order, full but the last
        want = ref[ref[:, 4] % shards == shard]                              # this shard's (pass, block) pairs in spiral order
        assert np.array_equal(p["blocks"][:, [0, 1, 2, 3, 4]].astype(np.int64), want.astype(np.int64))
        assert (p["blocks"][:, 5] == 0).all()
        seen += list(want[:, 4]); samples += p["samples"]
    assert sorted(seen) == list(range(len(ref)))
    assert samples == crop[2] * crop[3] * spp


def test_film_slots_of_passes_and_wavefront_entries(L, env):
    crop, bs = (3, 1, 50, 40), 16
    bc = 4 * 3
    p = plan(L, crop, 12, 4, bs, channels=7)
    ff = 50 * 40 * 7
    assert (p["film_floats"], p["n_slots"], p["pass_slots"]) == (ff, 3, 1)
    b = p["blocks"].astype(np.int64)
    pass_of = 2 - b[:, 4] // bc                                             # the spiral counts its passes down (spiral.cpp)
    assert np.array_equal(b[:, 6] + (b[:, 7] << 32), pass_of * ff)
    env.setenv("MTSAMD_PASS_SLOTS", "0")
    p = plan(L, crop, 12, 4, bs, channels=7)
    assert p["pass_slots"] == 0 and (p["blocks"][:, 6:] == 0).all()
    env.setenv("MTSAMD_PASS_SLOTS", "1")
    # wavefront streams: `split` entries per block, sample_base = sub * launch_spp, slot pass * split + sub
    env.setenv("MTSAMD_WAVEFRONT_SPLIT", "4")
    p = plan(L, crop, 16, 8, bs, wavefront=1)
    assert (p["split"], p["launch_spp"], p["n_slots"], p["n"]) == (4, 2, 8, 2 * bc * 4)
    b = p["blocks"].astype(np.int64)
    sub = np.tile(np.arange(4), 2 * bc)
    assert np.array_equal(b[:, 5], sub * 2)
    assert np.array_equal(b[:, 6] + (b[:, 7] << 32), ((1 - b[:, 4] // bc) * 4 + sub) * 50 * 40 * 5)
    assert p["samples"] == 50 * 40 * 16
    # slots beyond 2 GiB are not allocated: every entry adds to the one film
    env.delenv("MTSAMD_WAVEFRONT_SPLIT")
    p = plan(L, (0, 0, 8192, 8192), 4, 1, 1024)
    assert 4 * 8192 * 8192 * 5 * 4 > 2 << 30 and p["pass_slots"] == 0 and (p["blocks"][:, 6:] == 0).all()


@pytest.mark.parametrize("w,h,spp,cus", [(32, 32, 4096, 256), (256, 256, 64, 256), (1024, 1024, 64, 256), (100, 60, 48, 256), (64, 64, 1024, 32)])
def test_automatic_wavefront_split(L, env, w, h, spp, cus):
    split = 1
    while w * h * split < cus * 4096 and split * 2 <= spp and spp % (split * 2) == 0:
        split *= 2
    p = plan(L, (0, 0, w, h), spp, wavefront=1, cus=cus)
    assert (p["split"], p["launch_spp"], p["n_slots"], p["pass_slots"]) == (split, spp // split, split, int(split > 1))
    assert plan(L, (0, 0, w, h), spp, wavefront=0, cus=cus)["split"] == 1


def test_plan_errors(L, env):
    with pytest.raises(RuntimeError, match=r"sample_count \(6\) must be a multiple of samples_per_pass \(4\)\."):
        plan(L, (0, 0, 8, 8), 6, 4)
    with pytest.raises(RuntimeError, match="block_size too large"):
        plan(L, (0, 0, 8, 8), 4, block_size=1025)
    assert plan(L, (0, 0, 8, 8), 4, block_size=1024)["block_size"] == 1024 and plan(L, (0, 0, 8, 8), 4, block_size=5)["block_size"] == 8
    env.setenv("MTSAMD_WAVEFRONT_SPLIT", "3")
    with pytest.raises(RuntimeError, match="MTSAMD_WAVEFRONT_SPLIT must divide the sample count"):
        plan(L, (0, 0, 8, 8), 8, wavefront=1)
    assert plan(L, (0, 0, 8, 8), 8, wavefront=0)["split"] == 1           # a scene without wavefront streams does not split


# ---------------------------------------------------------------- calibration and the cost-sorted schedule
def test_lpt_policy(L):
    def pol(lpt, variant=11024, few=0, bs=32, launch_spp=512, n0=300, cus=256, stop=0):
        out = np.zeros(2, np.int64)
        call(L.rp_lpt_policy, lpt, variant, few, bs, launch_spp, n0, cus, stop, out)
        return int(out[0]), bool(out[1])
    assert pol(-1) == (4, False) and pol(-1, few=1) == (4, True) and pol(-1, launch_spp=256) == (2, False)
    assert pol(-1, n0=256) == (0, False) and pol(2, n0=256) == (4, False) and pol(3, n0=1) == (4, True)
    assert pol(-1, launch_spp=127) == (0, False) and pol(2, launch_spp=127) == (1, False) and pol(2, launch_spp=1) == (0, False)
    assert pol(0, few=1) == (0, True) and pol(1, few=1) == (4, False) and pol(3) == (4, True)
    assert pol(-1, variant=1) == (0, False) and pol(-1, bs=512) == (0, False) and pol(-1, stop=1) == (0, False) and pol(-1, cus=0, n0=2) == (4, False)


def test_calibration_blocks_are_the_distinct_positions(L):
    rows = [(64, 0, 32, 32, 7, 0, 5, 1), (0, 32, 32, 16, 3, 4, 9, 0), (64, 0, 32, 32, 19, 8, 2, 0), (0, 0, 32, 32, 1, 0, 0, 0)]
    out, n = np.zeros((4, 8), np.uint32), np.zeros(1, np.int64)
    call(L.rp_calibration_blocks, blocks_of(rows), 4, out, n)
    assert n[0] == 3
    assert out[:3].tolist() == [[0, 0, 32, 32, 1, 0, 0, 0], [0, 32, 32, 16, 3, 4, 0, 0], [64, 0, 32, 32, 7, 0, 0, 0]]


def test_smoothing_is_the_mean_over_measured_cells(L):
    """7 x 7 mean on the 4 x 4-pixel grid over the cells a calibration block measured, ragged border blocks included; tiles outside a
    block's pixels keep their raw measurement."""
    rng = np.random.default_rng(3)
    for crop, bs in [((5, 3, 70, 45), 16), ((0, 0, 61, 33), 32), ((2, 9, 13, 29), 8)]:
        x0, y0, w, h = crop
        cal = [(x0 + bx, y0 + by, min(bs, w - bx), min(bs, h - by), 0, 0, 0, 0) for by in range(0, h, bs) for bx in range(0, w, bs)]
        cal = sorted(cal, key=lambda b: (b[0], b[1]))
        cal = [b for k, b in enumerate(cal) if k % 5 != 2]                    # some blocks were not measured
        tpb = bs * bs // 16
        raw = rng.integers(0, 1 << 30, len(cal) * tpb).astype(np.uint64)
        gw, gh = (w + 3) // 4, (h + 3) // 4
        grid, where = np.full((gh, gw), -1.0), {}
        for k, b in enumerate(cal):
            for t in range(tpb):
                tx, ty = morton_origin(t)
                if tx < b[2] and ty < b[3]:
                    gx, gy = (b[0] - x0 + tx) // 4, (b[1] - y0 + ty) // 4
                    grid[gy, gx] = float(raw[k * tpb + t]); where[k * tpb + t] = (gx, gy)
        want = raw.copy()
        for s, (gx, gy) in where.items():
            win = grid[max(0, gy - 3):gy + 4, max(0, gx - 3):gx + 4]
            want[s] = np.uint64(int(win[win >= 0].sum() / (win >= 0).sum()))
        cost, pos, slot = raw.copy(), np.zeros(len(cal), np.uint64), np.zeros(len(cal), np.uint32)
        call(L.rp_smooth, cost, blocks_of(cal), len(cal), bs, np.array(crop, np.int32), pos, slot, 0, 1)
        assert np.array_equal(cost, want)
        assert pos.tolist() == [(b[0] << 32) | b[1] for b in cal] and slot.tolist() == [k * tpb for k in range(len(cal))]


def schedule(L, blocks, index, cost, bs, use_tiles, wg):
    b = blocks_of(blocks)
    pos = np.array([p for p, _ in index], np.uint64); slot = np.array([s for _, s in index], np.uint32)
    tiles, n = np.zeros(1 << 16, np.uint32), np.zeros(1, np.int64)
    call(L.rp_schedule, b, len(b), pos, slot, len(index), np.ascontiguousarray(cost, np.uint64), len(cost), bs, int(use_tiles), wg, len(tiles), tiles, n)
    return b, tiles[:n[0]]


def test_schedule_of_tiles_and_of_blocks(L):
    bs, tpb = 16, 16
    # spiral order: a full block, a ragged one (10 x 6 pixels: tiles with x0 < 10 and y0 < 6), a block never calibrated (costs 0)
    blocks = [(16, 0, 16, 16, 0, 0, 0, 0), (32, 0, 10, 6, 1, 0, 0, 0), (0, 0, 16, 16, 2, 0, 0, 0)]
    index = [((16 << 32) | 0, tpb), ((32 << 32) | 0, 0)]                        # sorted by position; block 0's costs start at slot 16
    cost = np.zeros(2 * tpb, np.uint64)
    cost[tpb:] = [5, 9, 5, 1, 9, 9, 0, 2, 7, 7, 7, 7, 3, 3, 3, 3]
    cost[:tpb] = np.arange(100, 116)
    _, tiles = schedule(L, blocks, index, cost, bs, True, 256)
    inside1 = [t for t in range(tpb) if morton_origin(t)[0] < 10 and morton_origin(t)[1] < 6]
    order = [(int(cost[tpb + t]), (0 << 12) | t) for t in range(tpb)] + [(100 + t, (1 << 12) | t) for t in inside1] + [(0, (2 << 12) | t) for t in range(tpb)]
    want = [code for _, code in sorted(order, key=lambda o: -o[0])]            # stable: ties in spiral order
    assert inside1 == [0, 1, 2, 3, 4, 6] and tiles[:len(want)].tolist() == want
    assert len(tiles) % 16 == 0 and (tiles[len(want):] == 0xFFFFFFFF).all() and len(tiles) - len(want) < 16
    _, tiles = schedule(L, blocks, index, cost, bs, True, 1024)
    assert len(tiles) == 64 and tiles[:len(want)].tolist() == want
    # whole blocks: sums over the tiles that hold a pixel, descending, ties in spiral order
    b, tiles = schedule(L, blocks, index, cost, bs, False, 256)
    assert len(tiles) == 0 and b[:, 4].tolist() == [1, 0, 2]
    b, _ = schedule(L, blocks + [(48, 0, 16, 16, 3, 0, 0, 0)], index, np.zeros(2 * tpb), bs, False, 256)
    assert b[:, 4].tolist() == [0, 1, 2, 3]


def test_schedule_falls_back_to_blocks_beyond_twenty_bits(L):
    n = 1 << 20
    blocks = np.zeros((n, 8), np.int64); blocks[:, 0] = np.arange(n) * 4; blocks[:, 2:4] = 4; blocks[:, 4] = np.arange(n)
    index = [((4 * k) << 32, k) for k in (7, 3)]
    cost = np.zeros(8, np.uint64); cost[3], cost[7] = 5, 9
    b, tiles = schedule(L, blocks, sorted(index), cost, 4, True, 256)
    assert len(tiles) == 0 and b[:3, 4].tolist() == [7, 3, 0] and b[3:, 4].tolist() == [k for k in range(1, n) if k not in (3, 7)]


# ---------------------------------------------------------------- the render switches
def switches(L):
    out = np.zeros(7, np.int64)
    call(L.rp_switches, out)
    return dict(zip(("kernel", "lean", "lpt", "lpt_debug", "pass_slots", "wavefront_split", "inject_lost_path"), out.tolist()))


def test_switches_accept_their_values(L, env):
    assert switches(L) == dict(kernel=-1, lean=1, lpt=-1, lpt_debug=0, pass_slots=1, wavefront_split=0, inject_lost_path=0)
    for value, variant in (("nested", 0), ("flat", 1), ("wga256", 10256), ("wga1024", 11024)):
        env.setenv("MTSAMD_KERNEL", value); assert switches(L)["kernel"] == variant
    for name, key, values in (("MTSAMD_LEAN", "lean", "012"), ("MTSAMD_LPT", "lpt", "0123"), ("MTSAMD_PASS_SLOTS", "pass_slots", "01")):
        for v in values:
            env.setenv(name, v); assert switches(L)[key] == int(v)
    env.setenv("MTSAMD_LPT_DEBUG", ""); assert switches(L)["lpt_debug"] == 1
    env.setenv("MTSAMD_WAVEFRONT_SPLIT", "16"); assert switches(L)["wavefront_split"] == 16
    env.setenv("MTSAMD_TEST_INJECT_LOST_PATH", "20000000"); assert switches(L)["inject_lost_path"] == 20000000
    env.setenv("MTSAMD_TEST_INJECT_LOST_PATH", "0"); assert switches(L)["inject_lost_path"] == 0


@pytest.mark.parametrize("name,value,message", [
    ("MTSAMD_KERNEL", "wga512", "MTSAMD_KERNEL must be one of nested, flat, wga256, wga1024"),
    ("MTSAMD_LEAN", "3", "MTSAMD_LEAN must be one of 0, 1, 2"), ("MTSAMD_LEAN", "", "MTSAMD_LEAN must be one of 0, 1, 2"),
    ("MTSAMD_LPT", "4", "MTSAMD_LPT must be one of 0, 1, 2, 3"), ("MTSAMD_LPT", "yes", "MTSAMD_LPT must be one of 0, 1, 2, 3"),
    ("MTSAMD_PASS_SLOTS", "2", "MTSAMD_PASS_SLOTS must be one of 0, 1"), ("MTSAMD_PASS_SLOTS", "off", "MTSAMD_PASS_SLOTS must be one of 0, 1"),
    ("MTSAMD_WAVEFRONT_SPLIT", "0", "MTSAMD_WAVEFRONT_SPLIT must be a positive integer"),
    ("MTSAMD_WAVEFRONT_SPLIT", "4x", "MTSAMD_WAVEFRONT_SPLIT must be a positive integer"),
    ("MTSAMD_TEST_INJECT_LOST_PATH", "-5", "MTSAMD_TEST_INJECT_LOST_PATH must be a non-negative integer"),
    ("MTSAMD_TEST_INJECT_LOST_PATH", "12ms", "MTSAMD_TEST_INJECT_LOST_PATH must be a non-negative integer"),
    ("MTSAMD_TEST_INJECT_LOST_PATH", "99999999999999999999999", "MTSAMD_TEST_INJECT_LOST_PATH must be a non-negative integer")])
def test_switches_reject_other_values(L, env, name, value, message):
    env.setenv(name, value)
    with pytest.raises(RuntimeError, match=message):
        switches(L)
    with pytest.raises(RuntimeError, match=message):                       # before any planning, whatever the scene
        plan(L, (0, 0, 8, 8), 4)


# ---------------------------------------------------------------- the kernel table and the choice of a scene's render kernel
MEDIA, NO_BVH, NO_SPHERE, NO_GRID_EVAL, NO_SHAPE_EMITTER, NO_PHASE_TREE, NO_RPV, HOMOG = (1 << k for k in range(8))      # dscene.h: MT_*
UNIT_A = MEDIA | NO_BVH | NO_SPHERE | NO_GRID_EVAL | NO_SHAPE_EMITTER | NO_PHASE_TREE | NO_RPV
UNIT_B = MEDIA | NO_BVH | NO_SPHERE | NO_SHAPE_EMITTER | NO_PHASE_TREE
FACTS = ("integrator", "spectral", "use_spectral_mis", "media", "bins", "srf", "srf_lookup_by_wavelength", "wavefront", "traits")


def kernel_table(L):
    rows, units, n_units = np.zeros((256, 6), np.int32), np.zeros((16, 2), np.int32), np.zeros(1, np.int32)
    n = L.rp_kernel_rows(rows, units, n_units)
    return [tuple(int(v) for v in r[:5]) + (bool(r[5]),) for r in rows[:n]], [(int(u), int(p)) for u, p in units[:n_units[0]]]


def choose(L, facts, block_size=32):
    facts = np.ascontiguousarray(facts, np.int32).reshape(-1, 9)
    out = np.zeros(len(facts), np.int32)
    call(L.rp_choose_kernel, facts, len(facts), block_size, out)
    return out


def choose_one(L, block_size=32, **f):
    facts = dict(integrator=kr.VOLPATH, spectral=0, use_spectral_mis=1, media=1, bins=0, srf=0, srf_lookup_by_wavelength=1, wavefront=0, traits=0)
    assert set(f) <= set(facts)
    facts.update(f)
    return int(choose(L, [facts[k] for k in FACTS], block_size)[0])


def test_kernel_table_lists_every_unit_once(L):
    rows, units = kernel_table(L)
    assert len(set(rows)) == len(rows) and sorted(u for u, _ in units) == list(range(8)) == sorted({r[0] for r in rows})
    assert [u for u, _ in units] == [kr.A, kr.B, kr.C, kr.H, kr.S, kr.P, kr.PS, kr.GENERAL]        # the order of preference
    promises = dict(units)
    assert promises[kr.GENERAL] == 0 and promises[kr.A] == UNIT_A and promises[kr.B] == promises[kr.S] == UNIT_B
    assert promises[kr.C] == UNIT_B & ~NO_BVH and promises[kr.H] == (UNIT_A & ~MEDIA & ~NO_RPV) | HOMOG
    assert promises[kr.P] == promises[kr.PS] == NO_BVH | NO_SPHERE | NO_RPV
    # a unit of the spectral build holds spectral rows only, and the other way round
    assert {r[0] for r in rows if r[5]} == {kr.GENERAL, kr.S, kr.PS} and {r[0] for r in rows if not r[5]} == {kr.GENERAL, kr.A, kr.B, kr.C, kr.H, kr.P}


def test_every_row_of_the_kernel_table_has_a_scene(L):
    assert set(kr.ROWS) == set(kernel_table(L)[0])


def test_choice_over_the_whole_input_space(L, env):
    """Every scene the choice can tell apart -- 3 integrators x 7 yes / no facts x 256 trait masks -- under every value of MTSAMD_KERNEL
    and MTSAMD_LEAN and block sizes 8 .. 64: the result is always a row of the table that serves the scene, every row is reached, a
    lean unit only ever renders a scene that keeps its promises, and a ring's paths divide the block."""
    rows, units = kernel_table(L)
    promises = dict(units)
    grid = np.stack(np.meshgrid(np.arange(3), *[np.arange(2)] * 7, np.arange(256), indexing="ij"), -1).reshape(-1, 9).astype(np.int32)
    assert len(grid) == 3 * 128 * 256
    integ, spectral, smis, wavefront, traits = grid[:, 0], grid[:, 1], grid[:, 2], grid[:, 7], grid[:, 8]
    reached, cases = set(), 0
    for kernel in (None, "nested", "flat", "wga256", "wga1024"):
        for lean in ("0", "1", "2"):
            env.setenv("MTSAMD_LEAN", lean)
            if kernel is None: env.delenv("MTSAMD_KERNEL", raising=False)
            else: env.setenv("MTSAMD_KERNEL", kernel)
            for bs in (8, 16, 32, 64):
                out = choose(L, grid, bs)
                unit, variant = kr.stat_unit(out), kr.stat_variant(out)
                cases += len(out)
                served = np.zeros(len(out), bool)
                for r in rows:
                    m = (unit == r[0]) & (variant == r[1]) & (integ == r[2]) & (spectral == r[5])
                    m &= (r[3] == kr.EITHER) | (smis == r[3])
                    m &= (r[4] == kr.EITHER) | (wavefront == r[4])
                    if m.any():
                        reached.add(r)
                    served |= m
                assert served.all(), (kernel, lean, bs, grid[~served][0], out[~served][0])
                if lean == "0":
                    assert (unit == kr.GENERAL).all()
                if lean == "2":
                    assert (unit != kr.A).all()
                for u, p in promises.items():
                    assert (traits[unit == u] & p == p).all(), (u, kernel, lean, bs)
                ringed = kr.is_ring(variant)
                assert ((bs * bs) % (variant[ringed] - kr.ring(0)) == 0).all()
    assert cases == 5 * 3 * 4 * 3 * 128 * 256 and reached == set(rows)


def test_choice_of_the_scenes_the_gpu_suite_names(L, env):
    """The kernels tests/test_gpu_parity.py expects of its scenes, from their facts alone."""
    one = lambda **f: choose_one(L, **f)
    c3 = dict(traits=UNIT_A)                                                                     # heterogeneous grey medium, every promise kept
    assert one(**c3) == 111024 == kr.stat(kr.ring(1024), kr.A)                                   # C3-like scene
    assert one(integrator=kr.VOLPATHMIS, **c3) == kr.stat(kr.ring(512), kr.A) == 110512          # volpathmis with spectral MIS on the same scene
    assert one(integrator=kr.VOLPATHMIS, use_spectral_mis=0, **c3) == 10512                      # ... without: no lean kernel
    assert one(media=0, traits=UNIT_A & ~MEDIA) == 0                                             # media-free volpath: nested per lane
    box = dict(integrator=kr.PATH, media=0, traits=NO_BVH | NO_SPHERE | NO_GRID_EVAL | NO_PHASE_TREE | NO_RPV)
    assert one(**box) == 400001                                                                  # Cornell `path`: the flat loop, unit p
    env.setenv("MTSAMD_LEAN", "0")
    assert one(**box) == 1 and one(**c3) == 11024
    env.setenv("MTSAMD_LEAN", "2")
    assert one(**c3) == 211024 and one(**box) == 400001
    env.delenv("MTSAMD_LEAN")
    assert one(spectral=1, traits=UNIT_B) == 310256                                              # spectral layered atmosphere: unit s
    assert one(spectral=1, integrator=kr.VOLPATHMIS, traits=UNIT_B) == 310256 and one(spectral=1, traits=UNIT_B & ~MEDIA) == 10256
    assert one(spectral=1, **box) == 500001                                                      # spectral `path` without BVH, spheres or rpv: unit ps
    assert one(spectral=1, **dict(box, traits=box["traits"] & ~NO_SPHERE)) == 1
    assert one(wavefront=1, **c3) == 11024                                                       # wavefront rgb volpath: the general 1024-path machine
    assert one(wavefront=1, integrator=kr.VOLPATHMIS, **c3) == 0                                 # wavefront volpathmis: nested
    assert one(wavefront=1, spectral=1, traits=UNIT_B) == 0 and one(wavefront=1, **box) == 400001
    # bins with a discrete response function that repeats a wavelength: nested; with distinct wavelengths on the machine
    assert one(spectral=1, bins=1, srf=1, srf_lookup_by_wavelength=0, traits=UNIT_B) == 0
    assert one(spectral=1, bins=1, srf=1, traits=UNIT_B) == 310256 and one(spectral=1, bins=1, srf=1, srf_lookup_by_wavelength=0, **box) == 500001
    assert one(block_size=16, traits=0) == 10256 and one(block_size=16, **c3) == 10256           # 16 x 16 blocks: 256 paths, general
    assert one(block_size=16, integrator=kr.VOLPATHMIS, **c3) == 10256 and one(block_size=8, **c3) == 1
    assert one(traits=UNIT_B) == 211024 and one(traits=UNIT_B & ~NO_BVH) == 711024               # rpv ground: b; a BVH: c
    assert one(media=1, traits=(UNIT_A & ~MEDIA & ~NO_RPV) | HOMOG) == 611024                    # homogeneous media: h
