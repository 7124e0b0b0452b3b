"""The env-step adjoint against the reference's autograd WHERE CLAMPS AND BRANCHES FIRE: the saturation / clamp fixtures of
oracle/gen_golden.py::gen_bptt (thrust clamp on both sides and on its ties, with and without motor lag, Euler and RK4; the rate
controller pushing single rotors into the clamps; the _ugly_fix clips of velocity, body rate and floor; the benchmark's 64-step
horizon with gate passes and re-spawns; NavigationEnv's reward branches on both sides; RK4 with per-agent drag coefficients).  tests/test_bptt_fixture_coverage.py shows, without a GPU, that each fixture is where it
claims to be.  Forward: rewards, done flags and the post-step state of every step bit for bit; gradient: the project's global bound
(test_bptt_gpu.REL_TOL of max|dL/da|) and a per-agent bound sized by the reference's own fp32 noise (check_action_gradients)."""
import pytest

from test_bptt_gpu import check_action_gradients

pytestmark = pytest.mark.gpu
MASK_CASES = ["bptt_racing_thrust_sat", "bptt_hover_thrust_sat_nodelay", "bptt_hover_thrust_sat_rk4", "bptt_hover_bodyrate_sat",
              "bptt_hover_state_clamps", "bptt_racing_thrust_h64", "bptt_nav_branches", "bptt_nav_rk4_drag"]


@pytest.mark.parametrize("name", MASK_CASES)
def test_action_gradients_match_reference_autograd_where_clamps_fire(name):
    check_action_gradients(name)
