"""materials = "through" of the denoisers on the GPU: bdpt_chain_kernel's guide keys feeding the
pack kernels of bdpt_denoise and bdpt_denoise_noise, against the existing numpy models fed the chain's
guides (tests/through_common.py).  Every comparison is on float32 bits; no tolerance.  33x25 is no
multiple of the wave or workgroup tiles."""
import pytest

from through_common import (MODEL_SCENES, PLAIN_SCENES, assert_cornell_partition, assert_matches_models,
                            assert_plain_scene_equals_diffuse, assert_refusals)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name,W,H", MODEL_SCENES)
def test_equals_the_models_fed_chain_guides(gpu, name, W, H):
    assert_matches_models(gpu, name, W, H)


@pytest.mark.parametrize("name,W,H", PLAIN_SCENES[:1])
def test_without_specular_spheres_in_view_it_is_diffuse(gpu, name, W, H):
    assert_plain_scene_equals_diffuse(gpu, name, W, H)


def test_cornell_differs_only_behind_its_balls(gpu):
    assert_cornell_partition(gpu)


def test_reproject_and_preview_refuse_it(gpu):
    assert_refusals(gpu)
