"""The learners' graph-replay driver leaves behind what each learner's own copy of it left.

``tests/test_gpu_deep.py`` and ``tests/test_gpu_gru.py`` compare k-iteration graphs with single replays of the same
driver; an error common to both would pass.  This test pins ``capture(iters_per_graph=4); iterations(9);
iteration(2)`` of DeepDQN and RecurrentDQN to ``tests/golden/learner_driver_parent_seeded.npz``: recorded on an
MI355X from this project's own commit 9a7cd56 (the last one where ``trainer/deep.py`` and ``trainer/recurrent.py``
each carried the warm-up, capture and replay dispatch) by ``tools/record_learner_driver_golden.py``, whose
``run_cases`` is what runs here -- its docstring has the command, the shapes and what each array is.  With
``epsilon = 0`` the counters, env state and replay contents do not depend on Q and must be equal bit for bit (they
repeated exactly between recordings); each parameter tensor's L2 norm, which depends on the order of float atomics,
to the tolerance tests/test_gpu_learners_dp.py uses for weight-dependent values."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "learner_driver_parent_seeded.npz")


def test_capture_and_replay_equal_the_recorded_parent(native_built):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import record_learner_driver_golden as rec

    g = np.load(GOLDEN)
    out = rec.run_cases()
    assert sorted(out) == sorted(g.files)
    assert int(g["deep_updates"]) == int(g["gru_updates"]) == 12 and int(g["gru_acts"]) == 11
    for k in sorted(out):
        print(k, out[k] if out[k].ndim == 0 else out[k].shape, g[k] if g[k].ndim == 0 else "")
        if rec.is_exact(k):
            assert out[k].dtype == g[k].dtype and np.array_equal(out[k], g[k]), k
        else:
            assert np.allclose(out[k], g[k], rtol=1e-4, atol=1e-5), (k, float(out[k]), float(g[k]))


@pytest.mark.parametrize("make", ["make_deep", "make_gru"])
def test_a_dropped_learner_frees_its_graphs_at_once(native_built, make):
    """No reference cycle between a learner and its driver: a learner that goes out of scope is freed there and
    then, graphs included.  Left to the cycle collector, a HIP graph can be destroyed in the middle of the next
    learner's capture (tests/test_gpu_learners_dp.py builds three in a row), which HIP refuses."""
    import gc
    import weakref

    import torch

    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import record_learner_driver_golden as rec

    d = getattr(rec, make)()
    d.capture(iters_per_graph=2)
    d.iterations(3)
    torch.cuda.synchronize()
    assert d._g_iter_k is not None
    ref = weakref.ref(d)
    gc.disable()
    try:
        del d
        assert ref() is None
    finally:
        gc.enable()
