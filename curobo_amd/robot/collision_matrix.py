"""The self-collision matrix of a robot: which link pairs the self-collision kernels must check.

Counterpart of the reference's ``RobotBuilder.compute_collision_matrix`` (``curobo/_src/robot/builder/builder_robot.py``
:417-502, 940-1172): neighbouring links are ignored, then ``custom_ignore``, then the link pairs that collide at the default
joint position (false positives of the sphere model), then -- optionally -- the link pairs that never collide over sampled
configurations.  The reference stores the distance of every sphere pair of a batch, ``[N, P]`` floats, and walks the link
pairs in a Python loop; here every batch is one FK launch and one ``link_pair_sweep`` launch (``csrc/link_pair_sweep.hip``)
that reduces the sphere pairs straight to two numbers per link pair, accumulated on the device over the batches and read
back once.
"""

from __future__ import annotations

from dataclasses import dataclass, field
from typing import Dict, List, Optional, Tuple

import numpy as np

from .loader import RobotModel, self_collision_pairs


def links_with_spheres(model: RobotModel) -> np.ndarray:
    """bool [L]: the link carries at least one sphere with radius >= 0 in ``model.link_spheres[0]``"""
    has = np.zeros(model.num_links, bool)
    enabled = model.link_spheres[0][:, 3] >= 0.0
    has[np.unique(np.asarray(model.link_sphere_idx_map, np.int64)[enabled])] = True
    return has


def neighbor_ignore(model: RobotModel) -> Dict[str, List[str]]:
    """``{link: [links]}`` of the parent-child neighbours: every link but the base ignores its parent in ``model.link_map`` and
    the parent ignores it, in link order (reference ``_create_neighbor_ignore_matrix``, builder_robot.py:940-963)."""
    names, out = model.link_names, {}
    for c in range(1, model.num_links):
        p = int(model.link_map[c])
        if p == c:
            continue
        for a, b in ((names[c], names[p]), (names[p], names[c])):
            if b not in out.setdefault(a, []):
                out[a].append(b)
    return out


def _ignored(ignore: Optional[Dict[str, List[str]]], a: str, b: str) -> bool:
    return bool(ignore) and (b in ignore.get(a, ()) or a in ignore.get(b, ()))


def link_pair_table(model: RobotModel, link_pairs: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """``(pair_locations [P, 2] int16, pair_group [P] int32)`` of the given link pairs ``[G, 2]`` (link indices): group g holds
    every sphere of link ``link_pairs[g, 0]`` against every sphere of link ``link_pairs[g, 1]`` -- disabled spheres included,
    the kernels skip them -- as ``(i, j)`` with ``i < j``, ordered by group, then ``(i, j)``."""
    sph_link = np.asarray(model.link_sphere_idx_map, np.int64)
    locs, grp = [], []
    for g, (a, b) in enumerate(np.asarray(link_pairs, np.int64).reshape(-1, 2)):
        sa, sb = np.nonzero(sph_link == a)[0], np.nonzero(sph_link == b)[0]
        ij = np.stack(np.meshgrid(sa, sb, indexing="ij"), -1).reshape(-1, 2)
        ij = np.sort(ij, axis=1)
        ij = ij[np.lexsort((ij[:, 1], ij[:, 0]))]
        locs.append(ij)
        grp.append(np.full(len(ij), g, np.int32))
    if not locs:
        return np.zeros((0, 2), np.int16), np.zeros((0,), np.int32)
    return np.concatenate(locs).astype(np.int16), np.concatenate(grp).astype(np.int32)


def candidate_link_pairs(model: RobotModel, ignore: Optional[Dict[str, List[str]]] = None) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """The link pairs a self-collision matrix has to decide on, with their sphere pairs.

    Returns ``(link_pairs [G, 2] link indices (a < b, lexicographic), pair_locations [P, 2] int16, pair_group [P] int32)``:
    every two different links that both carry at least one sphere with radius >= 0 in ``model.link_spheres[0]``, minus
    parent-child neighbours, minus the pairs of ``ignore`` (a pair listed in either direction counts, as in
    ``self_collision_pairs``).  Sphere pairs are ordered by group, then ``(i, j)``: every group is one contiguous run.

    Neighbour rule: two links are neighbours when one is the other's parent in ``model.link_map`` -- the reference's "child
    ignores parent, parent ignores child" (``neighbor_ignore``).  A link without spheres between two links with spheres is NOT
    walked past, whatever its joint: the reference's table lists ``panda_hand``-``panda_link8`` and ``panda_link8``-
    ``panda_link7`` but not ``panda_hand``-``panda_link7``, and that pair stays a candidate here too (it is decided by the
    default-position and sampling steps like every other pair).  This is what gives the packaged robots' candidate counts:
    ur10e 10, franka 46, dual_ur10e 81, unitree_g1 1128."""
    has = links_with_spheres(model)
    names = model.link_names
    links = np.nonzero(has)[0]
    pairs = []
    for x, a in enumerate(links):
        for b in links[x + 1:]:
            if int(model.link_map[b]) == a or int(model.link_map[a]) == b:
                continue
            if _ignored(ignore, names[a], names[b]):
                continue
            pairs.append((int(a), int(b)))
    link_pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    locs, grp = link_pair_table(model, link_pairs)
    return link_pairs, locs, grp


@dataclass
class SelfCollisionMatrix:
    """Result of ``compute_self_collision_matrix``.  ``max_penetration`` (metres, signed; ``-inf``: no valid sphere pair) and
    ``collision_count`` (configurations with a penetrating sphere pair) are per candidate link pair, over the swept
    configurations; ``num_samples`` is their number.  ``ignore`` is the ``self_collision_ignore`` table of a robot file."""

    link_pairs: List[Tuple[str, str]]
    max_penetration: np.ndarray
    collision_count: np.ndarray
    num_samples: int
    default_colliding: List[Tuple[str, str]]
    never_colliding: List[Tuple[str, str]]
    ignore: Dict[str, List[str]] = field(default_factory=dict)


def add_ignore(ignore: Dict[str, List[str]], model: RobotModel, a: str, b: str) -> None:
    """a new entry goes under the link that comes first in the model's link order"""
    if model.link_names.index(b) < model.link_names.index(a):
        a, b = b, a
    if b not in ignore.setdefault(a, []):
        ignore[a].append(b)


def merge_ignore(ignore: Dict[str, List[str]], custom: Optional[Dict[str, List[str]]]) -> None:
    """reference ``_merge_collision_ignore`` (builder_robot.py:965-972)"""
    for k, vs in (custom or {}).items():
        for v in vs:
            if v not in ignore.setdefault(k, []):
                ignore[k].append(v)


def assemble_matrix(model: RobotModel, link_pairs: np.ndarray, neighbors_and_custom: Dict[str, List[str]], default_count: np.ndarray,
                    max_penetration: np.ndarray, collision_count: np.ndarray, num_samples: int, prune_collisions: bool) -> SelfCollisionMatrix:
    """Steps three and four on the swept statistics: a candidate that penetrates at the default joint position is ``default_colliding``; of the others, one that penetrates at
    none of the ``num_samples`` configurations is ``never_colliding``.  The former always join ``ignore``, the latter when
    ``prune_collisions``."""
    names = model.link_names
    ignore = {k: list(v) for k, v in neighbors_and_custom.items()}
    named = [(names[a], names[b]) for a, b in link_pairs]
    default = np.asarray(default_count) > 0
    never = (~default) & (np.asarray(collision_count) == 0) if num_samples > 0 else np.zeros(len(named), bool)
    for g in np.nonzero(default)[0]:
        add_ignore(ignore, model, *named[g])
    if prune_collisions:
        for g in np.nonzero(never)[0]:
            add_ignore(ignore, model, *named[g])
    return SelfCollisionMatrix(named, np.asarray(max_penetration, np.float32), np.asarray(collision_count, np.int32), int(num_samples),
                               [named[g] for g in np.nonzero(default)[0]], [named[g] for g in np.nonzero(never)[0]], ignore)


def halton_configurations(model: RobotModel, n: int, sampler, joint_limit_margin: float):
    """the sampler's next ``n`` points scaled to the position limits widened by ``joint_limit_margin`` on both sides, in fp32
    as ``HaltonSeeds`` scales (``s * (high - low) + low``); torch tensor [n, dof] on the host"""
    import torch

    lo = torch.as_tensor(model.joint_limits_position[0], dtype=torch.float32) - joint_limit_margin
    hi = torch.as_tensor(model.joint_limits_position[1], dtype=torch.float32) + joint_limit_margin
    s = torch.as_tensor(sampler.random(n), dtype=torch.float32)
    return s * (hi - lo) + lo


def compute_self_collision_matrix(kinematics, num_samples: int = 1000, batch_size: int = 10000, seed: int = 345,
                                  custom_ignore: Optional[Dict[str, List[str]]] = None, prune_collisions: bool = True,
                                  joint_limit_margin: float = 0.1, samples=None) -> SelfCollisionMatrix:
    """The self-collision matrix of ``kinematics`` (a ``Kinematics`` with collision spheres), in the reference's order
    (builder_robot.py:474-500): neighbours, ``custom_ignore``, the link pairs that collide at ``default_joint_position``, then
    the link pairs that never collide over the samples.  The first three join ``ignore``; the fourth when ``prune_collisions``.

    ``num_samples`` batches of ``batch_size`` scrambled-Halton configurations are swept (``scipy.stats.qmc.Halton(dof,
    seed=seed)`` taken consecutively, scaled to the position limits widened by ``joint_limit_margin``); with ``samples``
    [M, dof] exactly those configurations instead, in batches of ``batch_size``.  Without ``samples`` and without
    ``prune_collisions`` nothing is sampled.  Every batch is one FK launch and one ``link_pair_sweep`` launch whose maxima and
    counts accumulate on the device; the host reads them once at the end, and no host loop runs over link pairs per batch.
    Limits of the sweep: at most 1024 spheres and 4096 candidate link pairs (``ValueError``)."""
    import torch

    from ..backends import geometry as geometry_hip

    model: RobotModel = kinematics.config.model
    kp = kinematics.kinematics_config
    dev = kp.device
    ignore0 = neighbor_ignore(model)
    merge_ignore(ignore0, custom_ignore)
    link_pairs, locs, grp = candidate_link_pairs(model, ignore0)
    G = len(link_pairs)
    if G == 0:
        return assemble_matrix(model, link_pairs, ignore0, np.zeros(0, np.int32), np.zeros(0, np.float32), np.zeros(0, np.int32), 0, prune_collisions)
    d_locs, d_grp = torch.as_tensor(locs, device=dev).contiguous(), torch.as_tensor(grp, device=dev).contiguous()
    pad = kp.self_collision.sphere_padding
    stats_f = torch.empty((2, G), dtype=torch.float32, device=dev)  # max penetration: default position, samples
    stats_i = torch.empty((2, G), dtype=torch.int32, device=dev)   # collision count: default position, samples

    def sweep(q, row: int, accumulate: bool) -> None:
        sph = kinematics.compute_kinematics(q.to(dev).contiguous()).robot_spheres
        geometry_hip.link_pair_sweep(stats_f[row], stats_i[row], sph, pad, d_locs, d_grp, G, accumulate=accumulate)

    sweep(kinematics.default_joint_position.view(1, -1), 0, False)
    total = 0
    if samples is not None:
        samples = torch.as_tensor(samples, dtype=torch.float32).reshape(-1, kp.num_dof)
        for k in range(0, samples.shape[0], int(batch_size)):
            q = samples[k:k + int(batch_size)]
            sweep(q, 1, total > 0)
            total += int(q.shape[0])
    elif prune_collisions:
        from scipy.stats.qmc import Halton

        sampler = Halton(d=kp.num_dof, seed=seed, scramble=True)
        for _ in range(int(num_samples)):
            sweep(halton_configurations(model, int(batch_size), sampler, joint_limit_margin), 1, total > 0)
            total += int(batch_size)
    if total == 0:
        stats_f[1].fill_(float("-inf"))
        stats_i[1].zero_()
    host = torch.cat([stats_f.view(torch.int32), stats_i]).cpu().numpy()  # the one read back
    return assemble_matrix(model, link_pairs, ignore0, host[2], host[1].view(np.float32), host[3], total, prune_collisions)


def collision_link_names(model: RobotModel) -> List[str]:
    """the links that carry spheres, in the order their spheres are laid out"""
    idx = np.asarray(model.link_sphere_idx_map, np.int64)
    _, first = np.unique(idx, return_index=True)
    return [model.link_names[int(idx[k])] for k in sorted(first)]


def pruned_collision_pairs(model: RobotModel, matrix: SelfCollisionMatrix) -> Tuple[np.ndarray, np.ndarray]:
    """``(collision_pairs [P', 2] int16, sphere_padding [S])`` of the model under ``matrix.ignore``, through
    ``self_collision_pairs``: what a robot file with that ``self_collision_ignore`` loads."""
    names = collision_link_names(model)
    idx = np.asarray(model.link_sphere_idx_map, np.int64)
    name_to_idx = {n: i for i, n in enumerate(model.link_names)}
    link_padding = {n: float(model.sphere_padding[np.nonzero(idx == name_to_idx[n])[0][0]]) for n in names}
    return self_collision_pairs(names, name_to_idx, matrix.ignore, link_padding, model.link_spheres[0], model.link_sphere_idx_map)
