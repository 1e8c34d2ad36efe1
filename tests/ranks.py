"""Ranks of the multi-rank GPU tests: N processes in one gloo group, sharing the visible GPUs.

Every rank opens the GPU it runs on, and so does the test process. A shared GPU host may limit how many processes hold
one GPU at a time, to as few as six. So by default at most ``RANKS_PER_GPU`` = 4 ranks share
one GPU, and a one-GPU run keeps five processes on the device (the test process and four ranks). A rank count that
needs more GPUs than are visible skips. On a host without such a limit, ``NFS_TEST_RANKS_PER_GPU=8`` runs the 8-rank
cases on one GPU (nine processes on it).

The ranks are started directly, with the environment torch.distributed.run gives a rank (RANK, LOCAL_RANK,
WORLD_SIZE, MASTER_ADDR / MASTER_PORT). Under that launcher its own process would hold the GPU open as well."""
import os
import socket
import subprocess
import time

import pytest

RANKS_PER_GPU = int(os.environ.get("NFS_TEST_RANKS_PER_GPU", "4"))


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def require_gpus_for(world):
    """skip (before any work) when the visible GPUs cannot hold ``world`` ranks at RANKS_PER_GPU per GPU"""
    import torch
    need, have = -(-world // RANKS_PER_GPU), torch.cuda.device_count()
    if have < need:
        pytest.skip("needs %d GPUs for %d ranks at %d ranks per GPU (NFS_TEST_RANKS_PER_GPU), found %d"
                    % (need, world, RANKS_PER_GPU, have))


def run_ranks(cmd, world, env, timeout):
    """run ``cmd`` as ranks 0..world-1; the first rank to fail stops the others.  Raises as ``subprocess.run(...,
    check=True, timeout=timeout)`` would"""
    port = str(free_port())
    procs, failed = [], None
    try:
        for r in range(world):
            e = dict(env, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(world), LOCAL_WORLD_SIZE=str(world),
                     MASTER_ADDR="127.0.0.1", MASTER_PORT=port)
            procs.append(subprocess.Popen(cmd, env=e))
        deadline = time.monotonic() + timeout
        while failed is None:
            codes = [p.poll() for p in procs]                   # (every rank, every pass)
            failed = next((p for p, c in zip(procs, codes) if c), None)
            if all(c is not None for c in codes):
                break
            if failed is None and time.monotonic() > deadline:
                raise subprocess.TimeoutExpired(cmd, timeout)
            time.sleep(0.1)
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
            p.wait()
    if failed is not None:
        raise subprocess.CalledProcessError(failed.returncode, cmd)
