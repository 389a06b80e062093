"""The fused trajectory launch (csrc/fused_device.hpp) gives the bits recorded in tests/golden/fused_chain_bits.npz on inputs in
which everything a workgroup reads per trajectory differs from row to row.

The fixture is not a reference's output: it holds what the build BEFORE the launch's load chain was shortened gave (the knots
requested with the state indices, dt / goal mode / state rows one trip later, dt and goal mode kept for the B-spline VJP, no
wrench gather for the points whose gradient no knot reads), under this compiler, on the inputs that
tests/golden/make_fused_chain_bits.py builds and refuses to record unless every case is what it is there for.  The other
fixtures and parity tests run one start state, one goal row, one dt and one goal mode, where a lane that reads another
trajectory's index, a dt taken from the wrong goal row or a goal mode that went stale between the forward pass and the VJP
changes nothing.  Here: Franka, the four-cuboid world, 5 trajectories, three start rows and two goal rows (different dt, one
implicit and one explicit goal) through unsorted index vectors; padded horizons 17 / 33 / 65 (1, 2 and 4 samples per knot
interval: as many leading points no knot's gradient reads) and 37 (no multiple of the knot intervals; one leftover point beside
the rows at 33, other splits at the others); the collision launch and the TERMS launch, each as compile-time shape and as the
generic kernel.  The comparison is exact, on the int32 view of every output word.

With a reuse memo of stride 1 the rows whose memo row has their bits must come back as the memo's sentinels, the rows whose memo
row differs in one word as evaluated -- the recorded bits again (both parities of the rows)."""

import importlib.util
import os

import numpy as np
import pytest

from conftest import GOLDEN_DIR

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location("make_fused_chain_bits", os.path.join(GOLDEN_DIR, "make_fused_chain_bits.py"))
M = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(M)

INPUTS, WANT = M.load()


def test_every_word_is_the_recorded_one():
    got = M.replay(INPUTS)
    assert sorted(got) == sorted(WANT) and len(WANT) == 2 * len(M.cases())
    for k in WANT:
        assert got[k].dtype == WANT[k].dtype == np.int32 and got[k].shape == WANT[k].shape, k
    differing = M.differing(got, WANT)
    print(f"{len(WANT)} arrays, {sum(v.size for v in WANT.values())} words, differing: {differing or 'none'}")
    assert not differing


@pytest.mark.parametrize("parity,word", [(0, "even"), (1, "odd")])
def test_memo_rows_are_copied_and_rows_one_word_off_are_evaluated(parity, word):
    bad = M.memo_differing(M.replay(INPUTS, memo=word), WANT, parity)
    print(f"memo rows of {word} parity copied, the others evaluated; differing: {bad or 'none'}")
    assert not bad
