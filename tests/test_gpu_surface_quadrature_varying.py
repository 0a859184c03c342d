"""The surface integrators on the device held to tests/surface_quadrature.py where something varies over a surface or over the sphere: checkerboard, grid
and bitmap textures (tex_color), lights whose emission depends on uv (mesh_emit_uv, mesh_emit_sampled: `-x hvs-light`, `-x texture-light`), the lat-long
environment map (env_eval, env_direct_pdf, env_sample_direction) and the light tree's emitter choice in direct and path (`-x ats`).  The quadrature writes
each from its definition in float64 and shares no shading code with the kernels or the oracle; a term that kernel and oracle both read wrongly from the
reference's text passes every bit-exact test and fails here.

The cases, their scenes, seeds, counts and the check are tests/surface_varying_cases.py's, the very list tests/test_surface_quadrature_varying.py runs on the
CPU oracle first; frame 24 x 18, K = 8 seeds, SE(r) <= 5 % and |mean(r) - 1| <= 4 SE(r) + the quadrature's error, at most 10 % of the pixels masked.

What the reference renderer computes and the published model does not is a named switch of the quadrature, held and told apart:
    sampled_emission_uv    a light sample reports Le(uv / |uv|), a ray that hits the light finds Le(uv): direct (0, 1), path under "emitter" and the light
                           tracer hold the first and miss the second, direct (1, 0) and path under "bsdf" hold the second, and the combinations hold
                           the two mixed by direct's power and path's balance heuristic
    grid_v_scale           the grid's v + scale_v
    sky_last_bin           a light sample of the map's last row or column leaves along the bin's lower edge
    path_emitting_side     a direction `path` samples finds a light lit on the side of its shading normal, light samples and `direct` on the side of its
                           geometric normal: on scenes.many_lights' tilted quads `path` under "bsdf" holds the shading side on the pixels where
                           the two differ and misses the one-sided reference there, and `path` under "all" is asserted to miss the one-sided
                           reference (its two-sided mix is not written); it is held under "all", tree on and off, on lights_over_floor instead
What each case reaches, on the oracle and on the device, is in profiles/surface_varying_note.md."""
import pytest

from tests import surface_varying_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def references(built):
    return C.References()


@pytest.fixture(scope="module")
def device(built):
    return C.Device()


@pytest.mark.parametrize("case", C.CASES, ids=C.CASE_IDS)
def test_device(references, device, case):
    C.run(case, device, references)
