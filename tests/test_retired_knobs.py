"""The step-plan variants that lost their A/B are gone (DESIGN.md "Appendix: environment knobs"): a value that used to
select one must fail loudly, not run the default plan under another name.  CPU-side: no GPU call is made."""
import os
import subprocess
import sys

import pytest

from conftest import ROOT

PKG = "multimodal_vae_comparison_amd"


def _python(code, **env):
    e = dict(os.environ)
    e.update(env)
    return subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=e, capture_output=True, text=True, timeout=300)


@pytest.mark.parametrize("knob, value, code", [
    # StreamPlan reads the variable when ops is imported
    ("MMVAE_STREAMS", "batch", f"import {PKG}.ops"),
    # trainer.capture reads the variable through this function, before it touches the GPU
    ("MMVAE_EARLY_ADAM", "4", f"from {PKG}.models import trainer; trainer.early_adam_from_env()"),
])
def test_retired_knob_values_raise(knob, value, code):
    r = _python(code, **{knob: value})
    assert r.returncode != 0, r.stdout + r.stderr
    last = r.stderr.strip().splitlines()[-1]
    assert last.startswith("ValueError") and knob in last, r.stderr


@pytest.mark.parametrize("knob, value, code, expect", [
    ("MMVAE_STREAMS", "0", f"from {PKG} import ops; print(ops.StreamPlan.enabled)", "False"),
    ("MMVAE_STREAMS", "tower", f"from {PKG} import ops; print(ops.StreamPlan.enabled)", "True"),
    ("MMVAE_EARLY_ADAM", "0", f"from {PKG}.models import trainer; print(trainer.early_adam_from_env())", "False"),
    ("MMVAE_EARLY_ADAM", "2", f"from {PKG}.models import trainer; print(trainer.early_adam_from_env())", "True"),
])
def test_kept_knob_values_are_accepted(knob, value, code, expect):
    r = _python(code, **{knob: value})
    assert r.returncode == 0, r.stderr
    assert r.stdout.split()[-1] == expect


def test_parked_weight_gradient_placement_knob_is_gone():
    """MMVAE_LINEAR_DW_LATER_AT has no reader left: not in the package, the tools or bench.py"""
    paths = [os.path.join(ROOT, "bench.py")]
    for top in (PKG, "tools"):
        for dirpath, _, files in os.walk(os.path.join(ROOT, top)):
            paths += [os.path.join(dirpath, f) for f in files if not f.endswith((".so", ".o", ".pyc"))]
    assert len(paths) > 50
    for p in paths:
        assert "MMVAE_LINEAR_DW_LATER_AT" not in open(p, errors="replace").read(), os.path.relpath(p, ROOT)
