#!/usr/bin/env python3
"""Record tests/golden/gru_seq_fwd_parent_seeded.npz, the fixture of
tests/test_gpu_gru_shared_bar.py::test_seq_fwd_equals_the_recorded_parent (1x MI355X).

The fixture pins the learner's forward, ``gru_seq_fwd_kernel``, to what it computed at commit 78d3a1e, the last one
at which the kernel carried its own copy of the bar (weight prologue, tile body, Q row).  It was recorded from a
built checkout of that commit:

    git worktree add /tmp/parent 78d3a1e && (cd /tmp/parent && python build.py)
    python tools/record_gru_seq_fwd_golden.py --root /tmp/parent tests/golden/gru_seq_fwd_parent_seeded.npz

``--root`` is the checkout whose package, kernels and test harness run (default: this one; recording from a later
commit pins that commit instead).  The case is one ``st_gru_seq_fwd`` launch through the harness of
tests/test_gpu_gru_learn_kernels.py: the packed nets ``_packed(11)`` (online) and ``_packed(12)`` (target) and
``gru_learn_refs.fwd_inputs(96, 3, "mixed", SEED)``.  B = 96 is three workgroups per net; S = 3 uses both parities of
the double-buffered LDS tiles, resets inside the run, the last step (no save) and ``HT`` blocks 0..2.  Stored per
output (``sv`` [5][S][B][256] and ``HT`` [S][B][256] as bf16 bits, ``Q`` and ``Qt`` [(S+1)B][4] fp32): the SHA-256
of its bytes and every 16th row; and ``in_sum``, sums of the inputs (x, h0, D, then the five packed arrays of each
net, as bit patterns where the array holds fp8 or bf16).
"""
import argparse
import hashlib
import os
import sys

import numpy as np

B, S, PATTERN, SEED = 96, 3, "mixed", 963
ROWS = slice(0, None, 16)
PACKED = ("whh8", "whhs", "wih", "bias4", "wq")


def sha(a) -> np.ndarray:
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), dtype=np.uint8).copy()


def rows(name: str, a) -> np.ndarray:
    """The output as rows: a unit row of ``sv`` / ``HT``, a sequence's [q0, q1, q2, 0] of ``Q`` / ``Qt``."""
    a = np.ascontiguousarray(a)
    return a.reshape(-1, 4 if name in ("Q", "Qt") else a.shape[-1])


def input_sums(inp, on, tg) -> np.ndarray:
    s = [float(np.asarray(inp[k], np.float64).sum()) for k in ("x", "h0", "D")]
    for pk in (on, tg):
        for n in PACKED:
            v = pk["b"][n].cpu()
            s.append(float((v if n in ("bias4", "wq") else v.long()).double().sum()))
    return np.array(s)


def run_case(T, R):
    """One launch of the case: (inputs' sums, {"sv", "HT", "Q", "Qt"}).  ``T`` is the module
    test_gpu_gru_learn_kernels, ``R`` is gru_learn_refs, both of the checkout that runs."""
    G, k = T._k()
    on, tg = T._packed(11), T._packed(12)
    inp = R.fwd_inputs(B, S, PATTERN, SEED)
    rc, sv, ht, Q, Qt = T._fwd_launch(G, k, inp, on, tg, B, S)
    assert rc == 0, rc
    return input_sums(inp, on, tg), {"sv": sv, "HT": ht, "Q": Q, "Qt": Qt}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    a = ap.parse_args()
    root = os.path.abspath(a.root)
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.join(root, "tests"))
    import gru_learn_refs as R
    import sharetrade
    import test_gpu_gru_learn_kernels as T
    for mod in (sharetrade, R, T):
        assert os.path.abspath(mod.__file__).startswith(root + os.sep), mod.__file__

    in_sum, out = run_case(T, R)
    rec = {"in_sum": in_sum}
    for name, v in out.items():
        r = rows(name, v)
        rec[name + "_sha256"], rec[name + "_rows"] = sha(r), r[ROWS].copy()
        print(name, r.dtype, r.shape, "sha256", bytes(rec[name + "_sha256"]).hex()[:16])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    np.savez_compressed(a.out, **rec)
    print("wrote", a.out, os.path.getsize(a.out), "bytes")
    return 0


if __name__ == "__main__":
    sys.exit(main())
