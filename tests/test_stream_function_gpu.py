"""Stylising through a stream function (grid variable 's') on the GPU: the test names and cases this file has
always had, on the checks that tests/test_source_variables_gpu.py writes once for the three kinds."""
import pytest

from tests import test_source_variables_gpu as V

pytestmark = pytest.mark.gpu
# (the update shapes this file has always run; the others: tests/test_source_variables_gpu.py)
UPDATE_SHAPES = [(2, 2, 2), (1, 4, 3), (4, 1, 1), (5, 6, 7), (9, 12, 10)]


@pytest.mark.parametrize("shape", V.KERNEL_SHAPES)
def test_forward_kernel_is_the_composition_bit_for_bit(shape):
    V.check_forward_kernel_is_the_composition_bit_for_bit("s", shape)


@pytest.mark.parametrize("shape", V.KERNEL_SHAPES)
def test_adjoint_kernel_is_the_composition_bit_for_bit(shape):
    V.check_adjoint_kernel_is_the_composition_bit_for_bit("s", shape)


def test_shapes_the_fused_advect_refuses_take_the_composition():
    V.check_shapes_the_fused_advect_refuses_take_the_composition("s")


@pytest.mark.parametrize("shape", UPDATE_SHAPES)
def test_update_kernel_gathers_the_transpose_and_applies_adam(shape):
    V.check_update_kernel_gathers_the_transpose_and_applies_adam("s", shape)


def test_gradient_parity_with_the_oracle_chain():
    V.check_gradient_parity_with_the_oracle_chain("s")


def test_step_is_adam_on_the_gradient_and_lowers_the_loss():
    V.check_step_is_adam_on_the_gradient_and_lowers_the_loss("s")


def test_graph_replay_reads_the_moved_variable_and_follows_the_eager_steps():
    V.check_graph_replay_reads_the_moved_variable_and_follows_the_eager_steps("s")


def test_dead_region_skipping_leaves_every_bit_of_the_update():
    V.check_dead_region_skipping_leaves_every_bit_of_the_update("s")


def test_order_2_runs_through_the_materialised_velocity():
    V.check_order_2_runs_through_the_materialised_velocity("s")


def test_the_flow_stays_divergence_free_and_a_free_velocity_does_not():
    V.check_the_flow_stays_divergence_free_and_a_free_velocity_does_not()


def test_two_ranks_sharing_the_views_keep_bit_identical_replicas(tmp_path):
    V.check_two_ranks_sharing_the_views_keep_bit_identical_replicas("s", tmp_path)


def test_styler_grid_optimises_a_stream_function_per_frame():
    V.check_styler_grid_optimises_the_variable_per_frame("s")
