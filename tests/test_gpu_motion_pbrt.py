"""A .pbrt scene that moves, end to end: parsed with the motion feature, uploaded, rendered by the motion build -- and bit for bit what the
same scene assembled with SceneBuilder renders."""
import numpy as np
import pytest

import motion_pbrt
from helpers import bits, pkg

pytestmark = pytest.mark.gpu


def test_pbrt_text_renders_what_the_builder_scene_renders(gpu_ctx):
    ctx = gpu_ctx
    ps = pkg.capi.ParsedScene(text=motion_pbrt.TEXT, motion_blur=True)
    ctx.upload(ps)
    assert ctx.kernel_set() == 4
    tile = (0, 0, 16, 16)
    a = ctx.radiance_samples(tile)
    ctx.upload(motion_pbrt.builder_scene())
    assert ctx.kernel_set() == 4
    b = ctx.radiance_samples(tile)
    assert (a > 0).any(-1).mean() > 0.15
    assert np.array_equal(bits(a), bits(b))
    # the scene does move: without its motion the picture is another one
    ps.motion = None
    ctx.upload(ps)
    assert ctx.kernel_set() == 0
    assert not np.array_equal(bits(ctx.radiance_samples(tile)), bits(a))
