"""Stylising through a velocity potential ('p') and the Helmholtz pair ('sp') on the GPU: the test names and cases this file has
always had, on the checks that tests/test_source_variables_gpu.py writes once for the three kinds."""
import pytest

from tests import test_source_variables_gpu as V

pytestmark = pytest.mark.gpu
KINDS = ["p", "sp"]


@pytest.mark.parametrize("shape", V.KERNEL_SHAPES)
@pytest.mark.parametrize("kind", KINDS)
def test_forward_kernel_is_the_composition_bit_for_bit(kind, shape):
    V.check_forward_kernel_is_the_composition_bit_for_bit(kind, shape)


@pytest.mark.parametrize("shape", V.KERNEL_SHAPES)
@pytest.mark.parametrize("kind", KINDS)
def test_adjoint_kernel_is_the_composition_bit_for_bit(kind, shape):
    V.check_adjoint_kernel_is_the_composition_bit_for_bit(kind, shape)


@pytest.mark.parametrize("kind", KINDS)
def test_shapes_the_fused_advect_refuses_take_the_composition(kind):
    V.check_shapes_the_fused_advect_refuses_take_the_composition(kind)


@pytest.mark.parametrize("shape", V.UPDATE_SHAPES)
@pytest.mark.parametrize("kind", KINDS)
def test_update_kernel_gathers_the_transpose_and_applies_adam(kind, shape):
    V.check_update_kernel_gathers_the_transpose_and_applies_adam(kind, shape)


@pytest.mark.parametrize("kind", KINDS)
def test_gradient_parity_with_the_oracle_chain(kind):
    V.check_gradient_parity_with_the_oracle_chain(kind)


@pytest.mark.parametrize("kind", KINDS)
def test_step_is_adam_on_the_gradient_and_lowers_the_loss(kind):
    V.check_step_is_adam_on_the_gradient_and_lowers_the_loss(kind)


@pytest.mark.parametrize("kind", KINDS)
def test_graph_replay_reads_the_moved_variable_and_follows_the_eager_steps(kind):
    V.check_graph_replay_reads_the_moved_variable_and_follows_the_eager_steps(kind)


@pytest.mark.parametrize("kind", KINDS)
def test_dead_region_skipping_leaves_every_bit_of_the_update(kind):
    V.check_dead_region_skipping_leaves_every_bit_of_the_update(kind)


@pytest.mark.parametrize("kind", KINDS)
def test_order_2_runs_through_the_materialised_velocity(kind):
    V.check_order_2_runs_through_the_materialised_velocity(kind)


@pytest.mark.parametrize("shape", V.DEGENERATE_SHAPES)
@pytest.mark.parametrize("kind", KINDS)
def test_velocity_is_zero_along_an_axis_of_length_1(kind, shape):
    V.check_velocity_is_zero_along_an_axis_of_length_1(kind, shape)


def test_transform_grad_is_the_reference_operator_and_differentiable():
    V.check_transform_grad_is_the_reference_operator_and_differentiable()


def test_the_potential_flow_stays_irrotational_and_a_free_velocity_does_not():
    V.check_the_potential_flow_stays_irrotational_and_a_free_velocity_does_not()


def test_the_helmholtz_velocity_is_the_sum_of_its_parts_and_both_move():
    V.check_the_helmholtz_velocity_is_the_sum_of_its_parts_and_both_move()


def test_two_ranks_sharing_the_views_keep_bit_identical_replicas(tmp_path):
    V.check_two_ranks_sharing_the_views_keep_bit_identical_replicas("p", tmp_path)


@pytest.mark.parametrize("kind", KINDS)
def test_styler_grid_optimises_the_variable_per_frame(kind):
    V.check_styler_grid_optimises_the_variable_per_frame(kind)


@pytest.mark.parametrize("kind", KINDS)
def test_styler_grid_starts_from_zero_without_an_init(kind):
    V.check_styler_grid_starts_from_zero_without_an_init(kind)
