"""examples/render_scene.c in its "radiance" mode: the C host renders its frame through rt_camera_rays and two calls
of rt_radiance (the second resuming the first's records) and finds rt_render's frame, bit for bit."""
import os
import subprocess

import numpy as np
import pytest

from tests.test_c_host import BIN, _params

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("n,side,spp", [(4, 23, 5), (7, 16, 1)])   # 32 triangles: brute force; 98: the BVH2 walk
def test_c_host_finds_its_frame_through_the_radiance_queries(tmp_path, n, side, spp):
    from ensem3a_openclraytracer_amd import workloads as W
    from ensem3a_openclraytracer_amd.scene import Scene
    assert os.path.exists(BIN), "examples/bin/render_scene is built by __graft_entry__.build()"
    text = W.grid_obj_text(n)
    sc = Scene.from_text(text, None, build_bvh=True, name=f"grid{n}")
    cam, env = sc.camera(side, side), sc.env()
    npix, mb = side * side, 4
    (tmp_path / "grid.obj").write_text(text)
    (tmp_path / "params.bin").write_bytes(_params(sc.materialData, cam, env, npix, spp, mb, W.ibl_preview()))
    prefix = str(tmp_path / "out")
    r = subprocess.run([BIN, str(tmp_path / "grid.obj"), str(tmp_path / "params.bin"), prefix, "radiance"],
                       capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stderr[-2000:]
    assert f"radiance queries of the camera rays: the same {npix} pixels" in r.stdout
    frame = np.fromfile(prefix + ".f32", np.float32)
    assert frame.size == 3 * npix and frame.mean() > 0.0
