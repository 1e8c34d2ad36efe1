"""libnfs_descent.so without a GPU: arguments are refused before any launch and reported through libnfs_hip.so's error channel
(what it exports, its version and its binding: tests/test_side_libraries_cpu.py)."""
from tests.test_side_libraries_cpu import _built


def test_arguments_are_refused_before_any_launch_and_reported_through_the_shared_channel():
    _l = _built()
    L, L0 = _l.side("descent"), _l.lib()
    E = _l.NFS_EINVAL
    # null pointers
    assert L.nfs_descent_step(None, 8, 4, 0.1, None) == E and b"nfs_descent_step: null pointer" in L0.nfs_last_error()
    assert L.nfs_advect_descent_fwd(8, 16, None, 0.1, 32, None, 4, 4, 4, None) == E
    assert b"nfs_advect_descent_fwd: null pointer" in L0.nfs_last_error()
    assert L.nfs_advect_descent_fwd(8, 16, 24, 0.1, None, None, 4, 4, 4, None) == E
    assert b"nfs_advect_descent_fwd: null pointer" in L0.nfs_last_error()
    assert L.nfs_advect2d_descent_fwd(None, 16, 24, 0.1, 32, 4, 4, None) == E
    assert b"nfs_advect2d_descent_fwd: null pointer" in L0.nfs_last_error()
    # an axis shorter than 2
    assert L.nfs_advect_descent_fwd(8, 16, 24, 0.1, 32, None, 4, 1, 4, None) == E and b"at least 2" in L0.nfs_last_error()
    assert L.nfs_advect2d_descent_fwd(8, 16, 24, 0.1, 32, 1, 9, None) == E and b"at least 2" in L0.nfs_last_error()
    # D * H * W >= 2^30
    assert L.nfs_advect_descent_fwd(8, 16, 24, 0.1, 32, None, 1 << 10, 1 << 10, 1 << 10, None) == E
    assert b"2^30" in L0.nfs_last_error()
    assert L.nfs_advect2d_descent_fwd(8, 16, 24, 0.1, 32, 1 << 15, 1 << 15, None) == E and b"2^30" in L0.nfs_last_error()
    # aliases, a negative count, a mask on a voxel count nfs_advect_fwd_live does not take
    assert L.nfs_advect_descent_fwd(8, 16, 24, 0.1, 16, None, 4, 4, 4, None) == E and b"alias" in L0.nfs_last_error()
    assert L.nfs_descent_step(8, 8, 4, 0.1, None) == E and b"alias" in L0.nfs_last_error()
    assert L.nfs_descent_step(8, 16, -1, 0.1, None) == E and b"negative" in L0.nfs_last_error()
    assert L.nfs_advect_descent_fwd(8, 16, 24, 0.1, 32, 40, 5, 6, 7, None) == E and b"multiple of 4" in L0.nfs_last_error()
