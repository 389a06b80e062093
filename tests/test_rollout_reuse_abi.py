"""The reuse entry points of the fused trajectory launches (``curobo_hip_rollout_trajectory_fused_reuse`` /
``curobo_hip_rollout_trajopt_fused_reuse``): declared, exported, additive (ABI version unchanged, the old symbols keep their
argument lists) and validated on the host before any launch -- no GPU needed."""

import ctypes as C
import re

import pytest

from curobo_amd import _lib

PLAIN, TERMS = "curobo_hip_rollout_trajectory_fused", "curobo_hip_rollout_trajopt_fused"
MEMO = ["memo_x", "memo_cost", "memo_grad", "memo_stride", "memo_slot"]


def _param_names(name):
    text = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER_PATH).read(), flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;{]*?)\)\s*;", text, flags=re.S)
    assert m, f"{name} is not declared in include/curobo_hip.h"
    return [re.findall(r"[A-Za-z_0-9]+", a)[-1] for a in m.group(1).split(",")]


def test_header_declares_and_library_exports_the_reuse_entry_points():
    lib = _lib.load()
    for base in (PLAIN, TERMS):
        assert base + "_reuse" in _lib.declared_symbols()
        assert hasattr(lib, base + "_reuse")
        old, new = _param_names(base), _param_names(base + "_reuse")
        # the same argument list plus the five reuse arguments in front of the stream
        assert new == old[:-1] + MEMO + ["stream"], (base, new)
    assert lib.curobo_hip_abi_version() == 7


def _call(name, **kw):
    """the entry point with NULL / 0 everywhere except a valid set of dimensions and ``kw``"""
    lib = _lib.load()
    names = _param_names(name)
    dims = dict(bspline_degree=3, sweep_steps=3, num_links=13, dof=7, padded_horizon=33, n_knots=12, link_chain_len=88,
                num_spheres=65, batch_size=8, num_envs=1)
    unknown = set(kw) - set(names)
    assert not unknown, unknown
    args = [kw.get(n, dims.get(n, 0 if t is C.c_int else None)) for n, t in zip(names, getattr(lib, name).argtypes)]
    return lib, getattr(lib, name)(*args)


@pytest.fixture(scope="module")
def host_word():
    """an address that is not NULL (validation fails before anything could read it)"""
    buf = (C.c_float * 4)()
    return C.addressof(buf), buf


BAD = [
    (dict(x=1, cost=0, grad=0), {}, b"all three or none"),
    (dict(x=1, cost=1, grad=0), {}, b"all three or none"),
    (dict(x=0, cost=0, grad=1), {}, b"all three or none"),
    (dict(x=1, cost=1, grad=1), dict(memo_stride=0), b"memo_stride must be >= 1"),
    (dict(x=1, cost=1, grad=1), dict(memo_stride=-4), b"memo_stride must be >= 1"),
    (dict(x=1, cost=1, grad=1), dict(memo_stride=4, memo_slot=4), b"memo_slot must be in [0, memo_stride)"),
    (dict(x=1, cost=1, grad=1), dict(memo_stride=4, memo_slot=-1), b"memo_slot must be in [0, memo_stride)"),
    (dict(x=1, cost=1, grad=1), dict(memo_stride=3, memo_slot=0), b"batch_size must be a multiple of memo_stride"),
    (dict(x=1, cost=1, grad=1), dict(memo_stride=4, out_position=1), b"materialised outputs"),
    (dict(x=1, cost=1, grad=1), dict(memo_stride=4, out_robot_spheres=1), b"materialised outputs"),
]


@pytest.mark.parametrize("name", [PLAIN + "_reuse", TERMS + "_reuse"])
@pytest.mark.parametrize("memo,extra,message", BAD)
def test_invalid_reuse_arguments_are_rejected_before_any_launch(name, memo, extra, message, host_word):
    addr = host_word[0]
    kw = {f"memo_{k}": (addr if v else None) for k, v in memo.items()}
    kw.update({k: (addr if k.startswith("out_") else v) for k, v in extra.items()})
    lib, rc = _call(name, **kw)
    assert rc == 1, (rc, lib.curobo_hip_last_error())
    err = lib.curobo_hip_last_error()
    assert message in err and name[len("curobo_hip_"):].encode() in err, err
    with pytest.raises(ValueError):
        _lib.check(rc)


@pytest.mark.parametrize("field", ["out_pose_distance", "out_position_distance", "out_rotation_distance", "out_goalset_idx",
                                   "out_cspace_cost"])
def test_reuse_is_refused_with_per_term_outputs(field, host_word):
    addr = host_word[0]
    terms = _lib.TrajOptTerms()
    setattr(terms, field, addr)
    lib, rc = _call(TERMS + "_reuse", memo_x=addr, memo_cost=addr, memo_grad=addr, memo_stride=4, terms=C.addressof(terms))
    assert rc == 1 and b"materialised outputs" in lib.curobo_hip_last_error()


@pytest.mark.parametrize("name", [PLAIN + "_reuse", TERMS + "_reuse"])
def test_valid_reuse_arguments_pass_validation(name, host_word):
    """an empty batch returns before the launch: every check above it has passed (stride 1 and a slot inside the stride too)"""
    addr = host_word[0]
    for stride, slot in ((4, 0), (4, 3), (1, 0)):
        lib, rc = _call(name, memo_x=addr, memo_cost=addr, memo_grad=addr, memo_stride=stride, memo_slot=slot, batch_size=0)
        assert rc == 0, lib.curobo_hip_last_error()
    lib, rc = _call(name, batch_size=0)  # no memo at all: the plain launch
    assert rc == 0, lib.curobo_hip_last_error()


def test_optimiser_switch_is_the_last_field_and_on_by_default():
    import dataclasses

    from curobo_amd.optim import LBFGSOptCfg

    fields = [f.name for f in dataclasses.fields(LBFGSOptCfg)]
    assert fields[-1] == "reuse_exploration_point" and LBFGSOptCfg().reuse_exploration_point is True
