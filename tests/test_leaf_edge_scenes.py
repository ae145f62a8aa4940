"""CPU check of the scenes of tests/leaf_edge_scenes.py: each special condition of the wide LEAF
step's triangle test (an exact zero, a denormal or an out-of-range determinant, an exact tie) is met
by at least one camera ray, computed in numpy fp32 in the kernels' operation order, and the oracle
renders every scene.  A scene that never reaches the branch proves nothing on the GPU."""
import numpy as np
import pytest

from leaf_edge_scenes import CHUNK, DEPTH, H, SEED, SPP, W, conditions, scenes

SCENES = scenes()


@pytest.mark.parametrize("name", ["degenerate", "huge", "ties"])
def test_camera_rays_meet_the_conditions(orc, name):
    objs, _, cam = SCENES[name]
    met = conditions(orc, name, objs, orc.camera_make(*cam))
    assert met, name
    for what, rays in met.items():
        assert rays > 0, f"{name}: no camera ray with {what}"


@pytest.mark.parametrize("name", sorted(SCENES))
def test_oracle_renders_the_scene(orc, name):
    objs, mats, cam = SCENES[name]
    nodes = orc.build_lbvh(objs, orc.morton_keys(objs), tight=True)
    rows = np.arange(H, dtype=np.int32)
    rgb, st = orc.render_sample(objs, mats, nodes, orc.camera_make(*cam), W, H, rows, SPP, DEPTH, SEED, CHUNK, nthreads=4)
    assert np.isfinite(rgb).all() and st.rays >= W * H * SPP and st.tri_tests > 0
    if name == "box":   # closed: paths bounce from wall to wall (a few leave through an edge's rounding)
        assert st.rays > W * H * SPP * DEPTH // 2
