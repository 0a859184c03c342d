"""The host sequence of the three beam-pass integrators (IntegratorPhotonBeams, IntegratorVirtualRayLights, IntegratorPhotonPlanes) in host/integrator.hpp,
checked without a device: tests/beam_pass_host_sequence_check.cpp runs each against stub rl_* functions, clean and with every ABI call failing in turn, as a
stand-alone program under the host's address and undefined-behaviour sanitizers (a leaked or twice-freed handle ends it with an error) — built and run as
tests/test_host_sequence.py builds and runs the check of the other light-pass integrators.  Nothing is loaded into Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_failure_releases_every_handle(tmp_path):
    exe = str(tmp_path / "beam_pass_host_sequence_check")
    build = subprocess.run(["g++", "-std=c++17", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                            os.path.join(ROOT, "tests", "beam_pass_host_sequence_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0 and not build.stderr, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "beam-pass host sequence: OK" in run.stdout and not run.stderr, run.stdout + run.stderr
