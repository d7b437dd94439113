"""Multi-process CPU harness: W gloo ranks on 127.0.0.1 via torch.multiprocessing."""
import os
import socket
import time
import traceback

import torch.multiprocessing as mp


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child_env(**kw):
    """Environment of a test's child process: the repo first on PYTHONPATH, the parent's entries KEPT after
    it (appended, not replaced -- a harness that injects its own path entries, e.g. to observe which native
    libraries the children load, must still see them), plus ``kw``."""
    pp = os.environ.get("PYTHONPATH", "")
    env = dict(os.environ, PYTHONPATH=ROOT + (os.pathsep + pp if pp else ""))
    env.update({k: str(v) for k, v in kw.items()})
    return env


def free_port() -> int:
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _entry(rank, world, port, fn, args, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank))
    try:
        res = fn(rank, world, *args)
        q.put((rank, "ok", res))
    except Exception:
        q.put((rank, "err", traceback.format_exc()))
    finally:
        import torch.distributed as dist
        if dist.is_initialized():
            dist.destroy_process_group()


def _end(procs):
    """Kill the ranks and wait until they are gone (a killed process may still hold its device)."""
    for p in procs:
        p.kill()
    for p in procs:
        p.join(30)


def _get(q, procs, deadline):
    """The next report; with a ``deadline`` a child that died without one or ran past it ends the run (all killed)."""
    while deadline is not None and q.empty():
        dead = [p.pid for p in procs if p.exitcode not in (None, 0)]
        if dead or time.monotonic() > deadline:
            _end(procs)
            raise AssertionError(f"children {dead} died without a report" if dead else "the ranks ran past their time limit")
        time.sleep(0.02)
    return q.get()


def run_ranks(fn, world, *args, timeout=300, limit=None):
    """``limit``: seconds all ranks together may take (GPU children: nothing may go on after a rank hung or died)."""
    ctx = mp.get_context("spawn")
    q = ctx.SimpleQueue()
    port = free_port()
    procs = [ctx.Process(target=_entry, args=(r, world, port, fn, args, q)) for r in range(world)]
    for p in procs:
        p.start()
    deadline = time.monotonic() + limit if limit is not None else None
    out = {}
    for _ in range(world):
        r, st, res = _get(q, procs, deadline)
        if st != "ok":
            _end(procs)
            raise AssertionError(f"rank {r} failed:\n{res}")
        out[r] = res
    for p in procs:
        p.join(timeout)
    return [out[r] for r in range(world)]
