"""float64 NumPy restatement of the link-pair sweep (``csrc/link_pair_sweep.hip``) and of the four-step self-collision matrix
(``curobo_amd/robot/collision_matrix.py``), written from their contracts and sharing no code with them."""

import numpy as np


def sweep_ref(spheres, padding, pair_locations, pair_group, n_groups, chunk=8):
    """``spheres`` [N, S, 4], ``padding`` [S], ``pair_locations`` [P, 2], ``pair_group`` [P] (every group one contiguous run) ->
    ``(max_penetration [G] f64, collision_count [G] int64, point_max [N, G] f64)``.

    penetration = (r_i + pad_i) + (r_j + pad_j) - |c_i - c_j|, all in float64 on the given values; a pair is valid when both
    padded radii are >= 0 (what ``pair_penetration`` of self_device.hpp sees); a group without a valid pair gives -inf / 0."""
    sph = np.asarray(spheres, np.float64).reshape(-1, np.shape(spheres)[-2], 4)
    N, G = sph.shape[0], int(n_groups)
    pl = np.asarray(pair_locations, np.int64).reshape(-1, 2)
    pg = np.asarray(pair_group, np.int64).reshape(-1)
    point_max = np.full((N, G), -np.inf)
    if len(pg):
        starts = np.concatenate([[0], np.nonzero(np.diff(pg))[0] + 1])
        present = pg[starts]
        assert len(np.unique(present)) == len(present), "every group must be one contiguous run"
        r = sph[:, :, 3] + np.asarray(padding, np.float64)[None]
        for n0 in range(0, N, chunk):
            c, rr = sph[n0:n0 + chunk, :, :3], r[n0:n0 + chunk]
            d = np.sqrt(((c[:, pl[:, 0]] - c[:, pl[:, 1]]) ** 2).sum(-1))
            ri, rj = rr[:, pl[:, 0]], rr[:, pl[:, 1]]
            pen = np.where((ri >= 0) & (rj >= 0), ri + rj - d, -np.inf)
            point_max[n0:n0 + chunk, present] = np.maximum.reduceat(pen, starts, axis=1)
    return point_max.max(axis=0) if N else np.full(G, -np.inf), (point_max > 0).sum(axis=0), point_max


def link_pairs_ref(model, ignore):
    """candidate link pairs [G, 2] (a < b) and their sphere-pair table: both links carry a sphere with radius >= 0, neither
    is the other's parent, and the pair is in ``ignore`` in neither direction"""
    sph_link = np.asarray(model.link_sphere_idx_map, np.int64)
    radius = model.link_spheres[0][:, 3]
    names = model.link_names
    carrying = [l for l in range(model.num_links) if (radius[sph_link == l] >= 0).any()]
    pairs, locs, grp = [], [], []
    for a in carrying:
        for b in carrying:
            if b <= a or model.link_map[b] == a or model.link_map[a] == b:
                continue
            if names[b] in ignore.get(names[a], []) or names[a] in ignore.get(names[b], []):
                continue
            sub = sorted((min(i, j), max(i, j)) for i in np.nonzero(sph_link == a)[0] for j in np.nonzero(sph_link == b)[0])
            locs += sub
            grp += [len(pairs)] * len(sub)
            pairs.append((a, b))
    return np.asarray(pairs, np.int64).reshape(-1, 2), np.asarray(locs, np.int16).reshape(-1, 2), np.asarray(grp, np.int32)


def matrix_ref(model, default_spheres, sample_spheres, custom_ignore=None, prune_collisions=True):
    """the four steps on given world-frame spheres (``default_spheres`` [1, S, 4] at the default joint position,
    ``sample_spheres`` [M, S, 4]): neighbours, ``custom_ignore``, default-colliding link pairs, never-colliding link pairs"""
    names = model.link_names
    ignore = {}

    def add(a, b):
        if b not in ignore.setdefault(a, []):
            ignore[a].append(b)

    for c in range(1, model.num_links):  # 1: child ignores parent, parent ignores child
        p = int(model.link_map[c])
        if p != c:
            add(names[c], names[p])
            add(names[p], names[c])
    for k, vs in (custom_ignore or {}).items():  # 2
        for v in vs:
            add(k, v)
    link_pairs, locs, grp = link_pairs_ref(model, ignore)
    G = len(link_pairs)
    named = [(names[a], names[b]) for a, b in link_pairs]  # (a < b: the first name is first in link order)
    _, d_count, _ = sweep_ref(default_spheres, model.sphere_padding, locs, grp, G)  # 3
    s_max, s_count, s_point = sweep_ref(sample_spheres, model.sphere_padding, locs, grp, G)  # 4
    default = d_count > 0
    never = ~default & (s_count == 0)
    for g in np.nonzero(default)[0]:
        add(*named[g])
    if prune_collisions:
        for g in np.nonzero(never)[0]:
            add(*named[g])
    return dict(link_pairs=named, link_pair_indices=link_pairs, pair_locations=locs, pair_group=grp, max_penetration=s_max,
                collision_count=s_count, point_max=s_point, default_colliding=[named[g] for g in np.nonzero(default)[0]],
                never_colliding=[named[g] for g in np.nonzero(never)[0]], ignore=ignore)
