"""`rustlight-amd ... virtual-ray-lights`: the argument errors the CLI reports before it opens a device (no GPU needed), the lines that parse, and
`vol-primitivies -p vrl`, which stays refused: the virtual ray lights have a subcommand of their own; and the new names in api.PUBLIC_SYMBOLS."""
from rustlight_amd import api
from tests import cli


def test_virtual_ray_lights_argument_errors(built, tmp_path):
    for args, word in ((("-r", "stratified:3", "virtual-ray-lights"), "stratified"),
                       (("--stream-mode", "per-sample", "virtual-ray-lights"), "per-sample"),
                       (("--numerics", "fast", "virtual-ray-lights"), "fast"),
                       (("--gpus", "2", "virtual-ray-lights"), "--gpus"),
                       (("-a", "3", "virtual-ray-lights"), "-a"),
                       (("-e", "3", "virtual-ray-lights"), "-e"),
                       (("--frames-in-flight", "2", "virtual-ray-lights"), "--frames-in-flight"),
                       (("virtual-ray-lights", "--nb-primitive", "0"), "--nb-primitive"),
                       (("virtual-ray-lights", "--nb-primitive", "12x"), "--nb-primitive"),
                       (("virtual-ray-lights", "--nb-primitive", str(api.BEAM_MAX + 1)), "--nb-primitive"),
                       (("virtual-ray-lights", "--radius", "0"), "--radius"),
                       (("virtual-ray-lights", "--radius", "-0.1"), "--radius"),
                       (("virtual-ray-lights", "--radius", "nan"), "--radius"),
                       (("virtual-ray-lights", "--radius", "inf"), "--radius"),
                       (("virtual-ray-lights", "--radius", "0.1x"), "--radius"),
                       (("virtual-ray-lights", "--light-streams", "other"), "--light-streams"),
                       (("virtual-ray-lights", "--tree-build", "device"), "--tree-build"),
                       (("virtual-ray-lights", "-p", "vrl"), "virtual-ray-lights option"),
                       (("virtual-ray-lights", "-s", "all"), "virtual-ray-lights option"),
                       (("--light-streams", "per-path", "virtual-ray-lights"), "after the subcommand"),
                       (("vol-primitivies", "-p", "vrl"), "not built")):
        cli.assert_refused(tmp_path, args, word)


def test_virtual_ray_lights_need_a_medium(built, tmp_path):
    r = cli.run_cli(tmp_path, "virtual-ray-lights", medium=())
    assert r.returncode == 2 and "needs a medium" in r.stderr and r.stderr.count("\n") == 1, r.stderr


def test_unknown_subcommand_lists_virtual_ray_lights(built, tmp_path):
    r = cli.run_cli(tmp_path, "virtual-ray-light")
    assert r.returncode == 2 and "`virtual-ray-lights`" in r.stderr and "`plane-single`" in r.stderr and r.stderr.count("\n") == 1, r.stderr


def test_virtual_ray_lights_options_parse_up_to_the_device(built, tmp_path):
    """Well-formed lines (-n parsed and ignored, both stream modes) get as far as opening a device: without one, the no-fallback refusal."""
    for args in (("virtual-ray-lights",), ("virtual-ray-lights", "--nb-primitive", "512", "--radius", "0.2", "-n", "3", "-m", "6", "-r", "inf"),
                 ("virtual-ray-lights", "--nb-primitive", "64", "--light-streams", "per-path"), ("virtual-ray-lights", "--light-streams", "reference", "-m", "inf")):
        cli.assert_reaches_device(tmp_path, args)


def test_the_new_names_are_public(built):
    import ctypes

    names = ("rl_vrl_map_build", "rl_vrl_map_build_words", "rl_vrl_map_info", "rl_vrl_map_read", "rl_vrl_map_destroy", "rl_render_vrl")
    so = ctypes.CDLL(api.LIB_PATH)
    for name in names:
        assert name in api.PUBLIC_SYMBOLS and hasattr(so, name), name
    for name in ("vrl_map", "vrl_map_from_words", "render_vrl"):
        assert callable(getattr(api.Context, name)), name
    assert issubclass(api.IntegratorVirtualRayLights, api._Integrator) and api.VrlMap._destroy == "rl_vrl_map_destroy"
