"""The recorder behind ``tests/test_launch_plan_cpu.py`` and ``tools/launch_identity.py``: every ``hip.ops`` wrapper
replaced by a function that notes its call, the device check and the stream queries stubbed, so that the engines build
and run whole forwards on CPU tensors.  Nothing is launched and nothing is computed; every tensor of a call stays alive
in the log, so addresses identify buffers."""
import collections
import types

import torch

from vdpp_amd.hip import ops
from vdpp_amd.models import common

Launch = collections.namedtuple("Launch", "name args kw")


def wrapper_names():
    """The ``hip.ops`` functions an engine may call (everything public but the two that touch no kernel)."""
    return [name for name in dir(ops)
            if isinstance(getattr(ops, name), types.FunctionType) and not name.startswith("_")
            and name not in ("zero_page", "last_error")]


def install(setattr_):
    """Replaces the wrappers and the stubs through ``setattr_(object, name, value)`` (``monkeypatch.setattr``, or the
    builtin for a process that ends with the run) and returns the list the launches are appended to."""
    launches = []

    def recorder(name):
        def f(*a, **k):
            launches.append(Launch(name, a, k))
            return 1024 if name.endswith("_bytes") else a[2] if name == "gemm" else None
        return f

    for name in wrapper_names():
        setattr_(ops, name, recorder(name))
    setattr_(common, "hip_device", lambda device, engine: torch.device(device))
    stream = types.SimpleNamespace(cuda_stream=0, synchronize=lambda: None)
    setattr_(torch.cuda, "current_stream", lambda *a, **k: stream)
    setattr_(torch.cuda, "is_current_stream_capturing", lambda: False)
    return launches
