"""libnfs_grid2d.so without a GPU: arguments are refused before any launch and reported through libnfs_hip.so's error channel
(what it exports, its version and its binding: tests/test_side_libraries_cpu.py)."""
from tests.test_side_libraries_cpu import _built


def test_arguments_are_refused_before_any_launch_and_reported_through_the_shared_channel():
    _l = _built()
    L, L0 = _l.side("grid2d"), _l.lib()
    assert L.nfs_advect2d_source_fwd(None, None, 0, None, 4, 4, None) == _l.NFS_EINVAL
    assert b"nfs_advect2d_source_fwd: null pointer" in L0.nfs_last_error()
    assert L.nfs_source2d_velocity_fwd(8, 4, 16, 4, 4, None) == _l.NFS_EINVAL and b"src 4" in L0.nfs_last_error()
    assert L.nfs_transport_step2d(8, 8, 1.0, 1.0, None, 0.0, 16, 1, 4, 1, None) == _l.NFS_EINVAL
    assert b"at least 2" in L0.nfs_last_error()
    assert L.nfs_advect2d_bwd_adam_fwd(8, 16, 24, 32, 40, None, 1 << 15, 1 << 15, 0.1, 0.9, 0.999, 1e-8, None) == _l.NFS_EINVAL
    assert b"2^30" in L0.nfs_last_error()
