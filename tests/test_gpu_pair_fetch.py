"""grid_fetch_pair (csrc/volpath_flat.h) on the smallest grids at which it can go wrong, bit for bit against the oracle.

The lookup of a heterogeneous medium on a pair grid issues its 16-byte gathers together, in pinned order, and waits for them once: the
first y-row of both z-levels always, the second y-rows unless every column of the grid holds the same profile (DMedium::pair_affine
bit 1), in which case the first rows stand in for them.  That flag never decides a value, so films and loop counters must equal the oracle's on

  * 2 x 2 x 2              every x0 is the first or the last column: the `hi0` / `hi1` selects and the clamp `min(x0, nx - 2)`
  * 8 x 1 x 1              one column, stored two voxels wide; all four rows of a cell are one row
  * 4 x 1 x 3              ny == 1 with columns that differ: the y-rows share their addresses although the flag is clear
  * 2 x 3 x 2, a profile   equal columns (flag set) with ny > 1: the second pair of rows is the first
  * 2 x 3 x 2, one voxel   the same grid with one voxel changed: flag clear
  * 3 x 2 x 5              odd sizes under a to_world with a projective row (world-to-local not affine: mat_point's division)
  * 3 x 2 x 5 rotated      the same grid under a rotated, affine to_world

(nz x ny x nx).  The medium fills a null-BSDF cube over a diffuse rectangle under a directional light; the sensor looks down on the whole
cube from close by, so that rays cross the last column and the last row of every grid and the half-voxel rim where the cell indices clamp.
Each case runs on lean unit a (the scene keeps its promises), on lean unit b and on the general unit -- the tracking step as
straight-line code (step_fast) and as medium_step -- at 32 x 32 pixels x 8 spp."""
import importlib

import numpy as np
import pytest

import tests.oracle_binding as ob

T = importlib.import_module("eradiate-kernel_amd.transform").ScalarTransform4f

BOX = T.translate([-2, -2, 0]) @ T.scale([4, 4, 2])            # the unit cube of grid space onto the medium's cube


def profile(nz, ny, nx):
    z = np.linspace(0.4, 1.9, nz, dtype=np.float32)
    return np.ascontiguousarray(np.broadcast_to(z[:, None, None], (nz, ny, nx)), dtype=np.float32)


def varied(nz, ny, nx, seed):
    return np.random.default_rng(seed).uniform(0.3, 2.0, (nz, ny, nx)).astype(np.float32)


def one_voxel_changed():
    g = profile(2, 3, 2)
    g[1, 2, 1] = np.float32(0.7)
    return g


def projective():
    m = BOX.matrix.astype(np.float64) @ np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0], [0.05, 0, 0.1, 1]], np.float64)
    return T(m.astype(np.float32))


GRIDS = {
    "2x2x2": (lambda: varied(2, 2, 2, 1), BOX, False),
    "8x1x1": (lambda: varied(8, 1, 1, 2), BOX, True),
    "4x1x3": (lambda: varied(4, 1, 3, 3), BOX, False),
    "2x3x2_profile": (lambda: profile(2, 3, 2), BOX, True),
    "2x3x2_one_voxel": (one_voxel_changed, BOX, False),
    "3x2x5_projective": (lambda: varied(3, 2, 5, 4), projective(), False),
    "3x2x5_rotated": (lambda: varied(3, 2, 5, 4), T.translate([0, 0, 1]) @ T.rotate([0.3, 0.5, 1.0], 25.0) @ T.translate([-2, -2, -1]) @ T.scale([4, 4, 2]), False),
}


def scene(name):
    make, to_world, _ = GRIDS[name]
    sigma_t = make()
    albedo = (0.95 - 0.3 * (sigma_t - sigma_t.min()) / max(float(sigma_t.max() - sigma_t.min()), 1e-6)).astype(np.float32)    # a profile where sigma_t is one
    medium = {"type": "heterogeneous", "scale": 1.0, "phase": {"type": "hg", "g": 0.5},
              "sigma_t": {"type": "gridvolume", "data": sigma_t, "to_world": to_world},
              "albedo": {"type": "gridvolume", "data": albedo, "to_world": to_world}}
    return {"type": "scene",
            "integrator": {"type": "volpath", "max_depth": -1, "rr_depth": 5, "block_size": 32, "samples_per_pass": -1},
            "sensor": {"type": "perspective", "to_world": T.look_at([0.3, -0.2, 8], [0, 0, 0], [0, 1, 0]), "fov": 40.0, "near_clip": 0.1, "far_clip": 100.0,
                       "film": {"type": "hdrfilm", "width": 32, "height": 32, "rfilter": {"type": "box"}},
                       "sampler": {"type": "independent", "sample_count": 8, "seed": 0}},
            "cloud": {"type": "cube", "to_world": T.translate([0, 0, 1]) @ T.scale([2, 2, 1]), "bsdf": {"type": "null"}, "interior": medium},
            "ground": {"type": "rectangle", "to_world": T.translate([0, 0, -0.01]) @ T.scale(6.0),
                       "bsdf": {"type": "diffuse", "reflectance": {"type": "rgb", "value": [0.5, 0.5, 0.5]}}},
            "sun": {"type": "directional", "direction": [0.5, 0.0, -0.866], "irradiance": 1.0}}


def check_grid(name):
    """the case is what its name says: the shape, and whether the grid is a z-profile (scene_host.cpp: grid_stats sets DVolume::columns_equal,
    hence DMedium::pair_affine bit 1, for exactly the grids whose columns are bitwise equal -- the library does not report the bit)"""
    make, to_world, is_profile = GRIDS[name]
    g = make()
    assert g.size >= 8 and name.startswith("x".join(str(n) for n in g.shape))
    assert bool((g == g[:, :1, :1]).all()) == is_profile, name
    if name.endswith("projective"):
        m = to_world.inverse().matrix
        assert m[3, 0] != 0 or m[3, 1] != 0 or m[3, 2] != 0        # world-to-local has a projective row: DVolume::affine == 0


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(GRIDS))
def test_pair_grid_lookups_match_the_oracle(gpu_rgb, monkeypatch, name):
    check_grid(name)
    d = scene(name)
    o = ob.OracleScene(d); ref = o.render(); so = o.last_stats
    assert ref[..., :3].max() > 0 and so["n_lookup"] > 8 * 32 * 32 // 4
    for lean_env, unit in ((None, 1), ("2", 2), ("0", 0)):
        if lean_env is None: monkeypatch.delenv("MTSAMD_LEAN", raising=False)
        else: monkeypatch.setenv("MTSAMD_LEAN", lean_env)
        s = gpu_rgb.load_dict(d)
        sensor = s.sensors()[0]
        assert s.integrator().render(s, sensor, collect_counters=True)
        gpu, st = np.array(sensor.film().bitmap(raw=True)), s.integrator().last_stats
        assert st["kernel_variant"] // 100000 == unit, (lean_env, st["kernel_variant"])
        assert np.array_equal(gpu, ref), (lean_env, float(np.abs(gpu - ref).max()))
        assert (st["n_iter"], st["n_lookup"], st["n_nee_step"], st["samples"]) == (so["n_iter"], so["n_lookup"], so["n_nee_step"], so["samples"])
