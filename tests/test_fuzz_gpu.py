"""Short runs of the randomised parity programs (tests/fuzz/conv_fuzz.py, ops_fuzz.py, model_fuzz.py, state_fuzz.py)
with fixed seeds: every convolution entry point over random shapes / layouts / storage types / tile
candidates against the CPU oracle, the element-wise / pooling / batch-norm / linear entry points, and
the model driver's state machine (no switch that only reschedules the arithmetic may change a bit; no property
switch, forward kind, held object or refusal may leave anything behind for the next call).
The long runs (minutes, other seeds) are started by hand; these keep the paths exercised in every run
of the suite.  Each tool exits non-zero with the failing case in its assertion message."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "fuzz"))
from state_fuzz import COMMITTED, PHRASE  # noqa: E402


def run_tool(name, *args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "fuzz", name), *args], cwd=ROOT,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, f"{name} {' '.join(args)}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
    return r.stdout


def test_conv_fuzz_short():
    out = run_tool("conv_fuzz.py", "--seconds", "8", "--seed", "101")
    assert "all within tolerance" in out


def test_ops_fuzz_short():
    out = run_tool("ops_fuzz.py", "--seconds", "5", "--seed", "102")
    assert "bit-exact" in out


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_model_fuzz_short(dtype):
    out = run_tool("model_fuzz.py", "--seconds", "8", "--seed", "103", "--dtype", dtype)
    assert "gave the pool's bits" in out


def test_defer_fuzz_short():
    """Random programs of the seven reference ops on a deferred context (folding and non-folding chains, reads,
    partial reads, rn_observe, writes into operands, frees, parameter updates; recorded and literal writes into
    parameters, the route switched off and on, the context destroyed mid-program) against the literal run."""
    out = run_tool("defer_fuzz.py", "--seconds", "10", "--seed", "104")
    assert "all within tolerance" in out
    kinds = [l for l in out.splitlines() if l.startswith("step kinds: ")]
    assert len(kinds) == 1, out
    ran = {k: int(v) for k, v in (item.split() for item in kinds[0][len("step kinds: "):].split(", "))}
    assert set(ran) == {"devparam", "toggle", "reopen"} and min(ran.values()) >= 1, ran


def test_view_fuzz_short():
    """Random fp32 entry points on views at random offsets of 0 / 4 / 8 / 12 bytes, guard bands always on
    (tests/views.py)."""
    out = run_tool("view_fuzz.py", "--seconds", "8", "--seed", "105")
    assert "all guards clean" in out


@pytest.mark.parametrize("arch,dtype,seed,steps", COMMITTED, ids=lambda v: str(v))
def test_state_fuzz_short(arch, dtype, seed, steps):
    """One model, one head of each kind, one neck and one pooler through property switches, every forward kind, held
    graphs and pipelines and the documented refusals: every output bit for bit what a never-reconfigured model gives,
    that model within the float64 bounds of the features' own tests.  The step counts give the coverage the tool
    asserts; tests/test_state_fuzz_host.py checks that on the CPU."""
    out = run_tool("state_fuzz.py", "--steps", str(steps), "--seed", str(seed), "--arch", arch, "--dtype", dtype)
    assert PHRASE in out
