"""fwd_entries_digest.py: one sha256 line per (forward entry, case, output buffer) of csrc/evc_lstm_fwd.hip - two builds of the library give the
same lines exactly when every entry computes the same bits.  The forward kernels use no atomics, so the digests repeat from run to run.

    [EVC_LIB=<other build>] [EVC_FORCE_TILE=k] python scripts/fwd_entries_digest.py

Needs the GPU (no CPU path).  Every entry of tests/_lstm_fwd_entries.py runs at T = 3: unplanned, each of its further forms, and - where it takes
a row plan - planned with rows_per_step = [32, 16, 0]: the plan ends before the last step, so the wavefront entries issue a launch in which
layer 0 has no rows left and layer 1 still has some.  EVC_FORCE_TILE is read once per process by the library: run once per forced value
(1..11) and once unforced.
"""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _lstm_fwd_entries as fe  # noqa: E402
from efficientvideoclassification_youtube8m_amd import ops  # noqa: E402

T, ROWS = 3, [32, 16, 0]


def main():
    ops.check_device(0)
    tile = os.environ.get("EVC_FORCE_TILE", "0") or "0"
    for name in fe.ENTRIES:
        cases = [("plain", {})] + [(v, dict(variant=v)) for v in fe.VARIANTS.get(name, ())]
        if name in fe.PLANNED:
            cases += [("planned", dict(rows=ROWS))] + [("planned " + v, dict(rows=ROWS, variant=v)) for v in fe.VARIANTS.get(name, ())]
        for label, kw in cases:
            call = fe.build(name, T=T, **kw)
            call.run()
            for buf, bits in call.bits().items():
                print("tile=%s %s [%s] %s %s" % (tile, name, label, buf, hashlib.sha256(bits.numpy().tobytes()).hexdigest()), flush=True)
    print("done")


if __name__ == "__main__":
    main()
