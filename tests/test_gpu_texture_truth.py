"""The device's filtered texture values against float64, with no oracle in between: a planar quad with a Mirror whose Kr is the
texture under test and one light of radiance 1 in every direction, so that the radiance of a camera sample is Kr as the device filtered
it with that ray's differentials (fs.scene_texture_truth).  The float64 side (test_texture_oracle.truth) computes the camera ray, the
offset rays, their hits, the uv differences, the mapping and the filtered value from the scene description, and first checks that it
reproduces the device's camera rays.

Which kernels evaluate Kr, as the launch code reads (pt_kernels.hip, ptk_shade and the recursion integrators):
  * rows under the constant infinite light ("env"): ptk_shade returns early for a scene with an infinite light and launches only
    k_shade_env (instances: k_shade_env_inst), before the material sort and the textured split; both call the __noinline__
    instantiation of pt_texture_calls.inc (value buffer in registers / scratch), as the recursion kernels of `whitted` and
    `directlighting` do.  These rows never reach k_tex_resolve.
  * rows inside the closed box of emitters ("box"), in world space, under `path`: no infinite light and no instance, so the textured
    hits go through k_tex_resolve -- the instantiation with PT_TEXN(x) = x##_inl, __forceinline__, value buffer in LDS -- and
    k_shade_general_res.  Every texture has such a row (test_truth_rows_are_pairwise checks it).
  * box rows with the quad as an instance: k_shade_general_inst (__noinline__).
The box rows run under `path` and `directlighting`: the reference's whitted integrator never adds the emission of a surface it hits.

Rows, columns and the pair count: fs.TEXTURE_TRUTH, test_texture_oracle.test_truth_rows_are_pairwise, truth_cases.  Each row may leave
out 3 % of its samples at most, on the device as on the oracle."""
import numpy as np
import pytest

import feature_scenes as fs
from test_texture_oracle import MAX_LEFT_OUT, observe, shared_noise_perm, truth_cases, truth_id

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", truth_cases(), ids=truth_id)
def test_device_texture_value_is_the_float64_one(gpu_ctx, case):
    """radiance = float64 value within bound(the float32 hit's error) + 8 * 2^-24 * value on every sample that is not left out."""
    row, integ = fs.TEXTURE_TRUTH[case[0]], case[1]
    gpu_ctx.upload(fs.scene_texture_truth(row, integ))
    excess, left, report = observe(gpu_ctx, row, integ, shared_noise_perm())
    print("texture truth [device %s]: left out %.2f %%, worst excess over the bound %.3g" % (truth_id(case), 100 * left, excess))
    assert excess <= 0.0, "beyond the bound by %.3g: %s" % (excess, report)
    assert left <= MAX_LEFT_OUT, "%.2f %% left out" % (100 * left)
