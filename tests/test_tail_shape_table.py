"""The compile-time shape table of the one-launch L-BFGS tail (csrc/tail_shapes.hpp) against the packaged Franka and the
solver configurations: a default that drifts away from its row would silently lose the specialised kernel (the dispatch
falls back to the run-time kernels).  Host-side queries only: no GPU, no allocation."""

import re

from conftest import load_model


def _trajopt_dims():
    from curobo_amd.solver.trajopt import TrajOptSolverCfg

    cfg, dof = TrajOptSolverCfg(), load_model("franka").num_dof
    opt_dim = cfg.rollout.n_knots * dof
    return dict(opt_dim=opt_dim, history=min(cfg.optimizer.history, opt_dim), n_linesearch=len(cfg.optimizer.line_search_scale), action_dim=dof)


def _ik_dims():
    from curobo_amd.solver.ik import IKSolverCfg

    cfg, dof = IKSolverCfg(), load_model("franka").num_dof
    return dict(opt_dim=dof, history=min(cfg.optimizer.history, dof), n_linesearch=len(cfg.optimizer.line_search_scale), action_dim=dof)


def test_solver_defaults_take_their_compile_time_shapes():
    from curobo_amd.backends.optimization import TAIL_ROW, TAIL_WAVE, TAIL_WORKGROUP, tail_form, tail_shape_id
    from curobo_amd.optim import LBFGSOptCfg

    t, ik = _trajopt_dims(), _ik_dims()
    assert t == dict(opt_dim=84, history=27, n_linesearch=4, action_dim=7) and tail_shape_id(**t) == 1
    assert ik == dict(opt_dim=7, history=7, n_linesearch=4, action_dim=7) and tail_shape_id(**ik) == 2
    d = LBFGSOptCfg()  # the optimiser's own defaults are the trajectory-optimisation ones
    assert (d.history, len(d.line_search_scale)) == (t["history"], t["n_linesearch"])
    # the forms the flagship workload and the solvers reach: between seed shards, single stream, IK rows
    assert tail_form(**t, batchsize=64, overlapped=True) == (TAIL_WAVE, 1)
    assert tail_form(**t, batchsize=256, overlapped=False) == (TAIL_WORKGROUP, 1)
    assert tail_form(**t, batchsize=1024, overlapped=False) == (TAIL_WAVE, 1), "past 512 problems: a wavefront each"
    assert tail_form(**ik, batchsize=2048, overlapped=False) == (TAIL_ROW, 2) == tail_form(**ik, batchsize=32, overlapped=True)


def test_no_shape_when_any_one_dimension_differs():
    from curobo_amd.backends.optimization import tail_form, tail_shape_id

    for dims in (_trajopt_dims(), _ik_dims()):
        for key in dims:
            for delta in (-1, 1):
                other = dict(dims, **{key: dims[key] + delta})
                assert tail_shape_id(**other) == 0, other
                assert tail_form(**other, batchsize=64, overlapped=True)[1] == 0, other
    assert tail_shape_id(84, 27, 4, 12) == 0 and tail_shape_id(7, 7, 4, 1) == 0
    assert tail_shape_id(72, 27, 4, 6) == 0, "a 6-dof arm"


def test_the_switch_turns_every_shape_off():
    from curobo_amd.backends.optimization import TAIL_ROW, TAIL_WAVE, set_tail_shapes_enabled, tail_form, tail_shape_id

    t, ik = _trajopt_dims(), _ik_dims()
    set_tail_shapes_enabled(False)
    try:
        assert tail_form(**t, batchsize=64, overlapped=True) == (TAIL_WAVE, 0)
        assert tail_form(**ik, batchsize=64, overlapped=False) == (TAIL_ROW, 0)
        assert tail_shape_id(**t) == 1, "the table itself does not depend on the switch"
    finally:
        set_tail_shapes_enabled(True)
    assert tail_form(**t, batchsize=64, overlapped=True) == (TAIL_WAVE, 1)


def test_lane_offsets_past_31_bits_take_the_64_bit_kernels():
    """batch * opt_dim * 4 >= 2^31: no 32-bit lane offset can hold a row's place.  The row form falls back to the plain
    kernel, the workgroup form to the wavefront form (whose problem index lives in the scalar base)."""
    from curobo_amd.backends.optimization import TAIL_PLAIN, TAIL_ROW, TAIL_WAVE, TAIL_WORKGROUP, tail_form

    ik, t = _ik_dims(), _trajopt_dims()
    edge = (1 << 31) // (4 * ik["opt_dim"]) + 1  # first batch with batch * opt_dim * 4 >= 2^31
    assert edge * ik["opt_dim"] * 4 >= 1 << 31 > (edge - 1) * ik["opt_dim"] * 4
    assert tail_form(**ik, batchsize=edge, overlapped=False) == (TAIL_PLAIN, 0)
    assert tail_form(**ik, batchsize=edge, overlapped=True) == (TAIL_PLAIN, 0)
    # the row form's own bound is tighter: the candidate rows are [batch][n_linesearch][opt_dim]
    fits = ((1 << 31) - 1) // (4 * ik["opt_dim"] * ik["n_linesearch"])
    assert tail_form(**ik, batchsize=fits, overlapped=False) == (TAIL_ROW, 2)
    assert tail_form(**ik, batchsize=fits + 1, overlapped=False) == (TAIL_PLAIN, 0)
    assert tail_form(1, 0, 1, 1, (1 << 29) - 1, False) == (TAIL_ROW, 0) and tail_form(1, 0, 1, 1, 1 << 29, False) == (TAIL_PLAIN, 0)
    # wavefront-sized problems: always a 64-lane form, with its shape (the workgroup form needs batch <= 512 anyway)
    big = (1 << 31) // (4 * t["opt_dim"]) + 1
    assert tail_form(**t, batchsize=big, overlapped=False) == (TAIL_WAVE, 1) == tail_form(**t, batchsize=big, overlapped=True)
    assert tail_form(**t, batchsize=512, overlapped=False) == (TAIL_WORKGROUP, 1)


def test_table_rows_are_consistent_with_the_source():
    import os

    from curobo_amd.backends.optimization import tail_shape_id
    from curobo_amd.build import CSRC, HEADERS

    assert "tail_shapes.hpp" in HEADERS
    text = open(os.path.join(CSRC, "tail_shapes.hpp")).read()
    rows = re.findall(r"#define CUROBO_TAIL_SHAPE_(\d+) TailShape<(\d+), (\d+), (\d+), (\d+)>", text)
    assert [int(r[0]) for r in rows] == list(range(1, len(rows) + 1))
    assert int(re.search(r"#define CUROBO_TAIL_NUM_SHAPES (\d+)", text).group(1)) == len(rows)
    for k, v, m, nls, ad in rows:
        assert tail_shape_id(int(v), int(m), int(nls), int(ad)) == int(k)
