"""GPU: the library's own sharded grouped search (tsh_search_sharded_grouped) with MORE THAN ONE rank: over the host
transport (tsh_comm_create_host + gloo) at world 2 and 3, and over the RCCL branch at world 2 against tests/fake_rccl
(real RCCL refuses two ranks on one device, and a test box has one GPU).  tests/_shard_grouped_worker.py holds the checks:
against the oracle and against one un-sharded tsh_search_grouped, groups that span every rank, a mask by pointer and by
handle, the overflow retry, 20 queries in shrinking groups and never batched, TSH_OPT_EXCHANGE_AHEAD set and ignored, a bad
groups handle as a local failure, out_group on slice owners and non-owners.  Here: every rank passed every check, and
every rank got the same bytes.  At most three GPU processes run at once, each under its own time limit."""
import os
import re
import socket
import subprocess
import sys
import tempfile

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "_shard_grouped_worker.py")
ROWS = "6000"
CHECKS = 11  # lines that end in " ok" per rank


def _port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _verdict(out, world):
    assert "MISMATCH" not in out, out[-4000:]
    assert out.count(" ok\n") == world * CHECKS, out[-4000:]
    digests = re.findall(r"rank (\d+) digest ([0-9a-f]{64})", out)
    assert sorted(int(r) for r, _ in digests) == list(range(world)), out[-4000:]
    assert len({h for _, h in digests}) == 1, "the ranks' answers differ: %r" % (digests,)


@pytest.mark.parametrize("world", [2, 3])
def test_sharded_grouped_over_host_transport(hip_lib, world):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world),
           "--master-addr", "127.0.0.1", "--master-port", str(_port()), WORKER, ROWS, "host"]
    p = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    out = p.stdout + p.stderr
    assert p.returncode == 0, out[-4000:]
    _verdict(out, world)


def test_sharded_grouped_over_the_rccl_branch(hip_lib):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import fake_rccl

    world, lib = 2, fake_rccl.build()
    with tempfile.TemporaryDirectory() as tmp:
        env = dict(os.environ, WORLD_SIZE=str(world), TSH_RCCL_LIB=lib, TSH_FAKE_RCCL_TIMEOUT_S="120", OMP_NUM_THREADS="2",
                   HSA_ENABLE_IPC_MODE_LEGACY="0")
        procs = [subprocess.Popen([sys.executable, WORKER, ROWS, "rccl", os.path.join(tmp, "uid")], cwd=ROOT,
                                  env=dict(env, RANK=str(r), LOCAL_RANK="0"), stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                                  text=True) for r in range(world)]
        outs, rcs = [], []
        try:
            for p in procs:  # every process has its own time limit; the first failure ends the others
                outs.append(p.communicate(timeout=300)[0])
                rcs.append(p.returncode)
                if p.returncode != 0:
                    break
        finally:
            for p in procs:  # exactly the processes started above
                if p.poll() is None:
                    p.kill()
                    p.wait()
    out = "\n".join(outs)
    assert rcs == [0] * world, out[-6000:]
    _verdict(out, world)
