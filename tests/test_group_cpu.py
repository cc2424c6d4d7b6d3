"""Index groups without a kernel launch: the argument checks of cls_db_group_create and cls_place_batch_group, on any
machine (with no GPU visible the group create fails as cls_db_create does)."""
import ctypes as C

import numpy as np
import pytest

from classeq2_amd import _abi, engine
from classeq2_amd.synth import SynthDb


def test_group_create_checks_devices_first():
    s = SynthDb(30, 200, 6, 3)
    n_dev = engine.device_count()
    with pytest.raises(engine.ClsError) as e:
        engine.PlacementDbGroup(s.flat, [0, n_dev + 3])
    if n_dev == 0:  # no device: the message of cls_db_create
        with pytest.raises(engine.ClsError) as e1:
            engine.PlacementDb(s.flat, device=0)
        assert e.value.code == e1.value.code == -4
        assert e.value.msg.split(": ", 1)[1] == e1.value.msg.split(": ", 1)[1]
    else:
        assert e.value.code == -1 and "out of range" in e.value.msg


def test_group_null_arguments():
    L = engine.lib()
    assert L.cls_db_group_create(None, None, 0, None) == -1
    assert L.cls_db_group_size(None, C.byref(C.c_uint32())) == -1
    assert L.cls_db_group_replica(None, 0, C.byref(C.c_void_p())) == -1
    out = np.zeros(1, dtype=_abi.PLACEMENT_DTYPE)
    off = np.array([0, 4], dtype=np.uint64)
    assert L.cls_place_batch_group(None, b"ACGT", off.ctypes.data, 1, None, out.ctypes.data, None) == -1
    assert L.cls_place_sequences_group(None, None, b"-", b"x", None, 0, 0, None, None) == -1
    L.cls_db_group_destroy(None)
