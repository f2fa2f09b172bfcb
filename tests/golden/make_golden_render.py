"""tests/golden/render.npz: what the numpy oracle (tests/render_oracle.py, float64 setup + integer raster) gives for the two fixed scenes of
tests/test_render.py.  Nothing is recorded from the reference: its renderer (pyrender + EGL) cannot run where this package is developed.

    python -m tests.golden.make_golden_render

  adv_id   int32 [2,40,72]      id images of the adversarial scene, 2 views (scene-space triangles: both views show the same picture)
  e2e_id   int32 [3,4,96,128]   id images of the end-to-end clip (ellipsoid body, box, ground; T = 3, past_len = 1, 4 views)
  e2e_rgb  uint8 [3,4,96,128,3]
  e2e_share32  float64 [12]     share of pixels per image that differ when the SETUP stage is restated in float32 instead of float64
The conditions the tests rely on are asserted here and again by the tests."""
import os
import numpy as np
from tests import render_oracle as ro

HERE = os.path.dirname(os.path.abspath(__file__))
ADV = dict(H=40, W=72, views=2)
E2E = dict(H=96, W=128, views=4, T=3, past_len=1)
CAP = 0.005                        # differing pixels per image allowed between the kernel and the float64 oracle


def adversarial():
    scene = ro.make_scene(bg=(0.2, 0.3, 0.4))
    return scene, [ro.adversarial_scene(scene, ADV['H'], ADV['W'], seed=0)]


def end_to_end():
    c = ro.e2e_clip(E2E['T'])
    scene, meshes = ro.clip_scene(c['body'], c['body_face'], c['obj'], c['obj_face'], E2E['past_len'])
    return c, scene, meshes


def e2e_share32(o64, scene, meshes):
    o32 = ro.render(scene, meshes, E2E['T'], E2E['views'], E2E['H'], E2E['W'], ft=np.float32)
    return (o64[2] != o32[2]).any(-1).reshape(E2E['T'] * E2E['views'], -1).mean(1)


def main():
    scene, meshes = adversarial()
    adv = ro.render(scene, meshes, 1, ADV['views'], ADV['H'], ADV['W'])
    assert adv[4] == 0 and len(np.unique(adv[0])) > 25
    c, scene, meshes = end_to_end()
    o64 = ro.render(scene, meshes, E2E['T'], E2E['views'], E2E['H'], E2E['W'])
    share = e2e_share32(o64, scene, meshes)
    print('float32 setup vs float64 setup, differing pixel share per image:', share)
    assert o64[4] == 0 and share.max() <= CAP / 4
    np.savez_compressed(os.path.join(HERE, 'render.npz'), adv_id=adv[0][0], e2e_id=o64[0], e2e_rgb=o64[2], e2e_share32=share)


if __name__ == '__main__':
    main()
