"""Flip the kernel library's A/B switches (ND_ATTN_*, ND_DKDV_BQ, ND_WGRAD_VARIANT, ND_WGRAD_PLAN, ND_CE) inside a test.

The library parses them into plain globals when it is loaded, which in a test session happens once, in the first
``hip_lib`` fixture: setting the variable afterwards selects nothing.  ``switches(...)`` sets the variables, has the
library parse the environment again (``nd_env_reload``), and asserts through ``nd_env_describe`` that every value it
was asked for is the parsed state; on exit it restores the environment and reloads once more.

    with switches(ND_ATTN_FWD="r", ND_ATTN_DKDV_NB=None):   # None: unset (the default, nothing to assert)
        ...
"""
import contextlib
import ctypes
import os

from nanodiloco_amd.ops import _ext


def describe() -> dict:
    """The parsed switch state of the loaded library, {name: value as text}."""
    buf = ctypes.create_string_buffer(1024)
    n = _ext.lib().nd_env_describe(buf, len(buf))
    assert 0 < n < len(buf), n
    return dict(tok.split("=", 1) for tok in buf.value.decode().split())


def _spelled(value: str) -> str:
    return value if value != "" else "default"  # an empty ND_WGRAD_VARIANT is the default kernel


@contextlib.contextmanager
def switches(**env):
    saved = {k: os.environ.get(k) for k in env}
    try:
        for k, v in env.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = str(v)
        assert _ext.lib().nd_env_reload() == 0
        state = describe()
        for k, v in env.items():
            if v is not None:
                assert k in state, f"{k} is not a switch the library describes: {sorted(state)}"
                assert state[k] == _spelled(str(v)), f"switch {k}={v!s} did not take: the library runs {k}={state[k]}"
        yield state
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        _ext.lib().nd_env_reload()
