"""The float64 frustum flags of tests/mapper_decay_ref.py against the reference's own ``mark_blocks_in_frustum_kernel``
(perception/mapper/kernel/builder/builder_decay.py, unmodified), run thread by thread in fp32 through tests/golden/warp_emulator,
on the decay tests' scene: every block of the grid as an allocated block, for the frustum test's two cameras and the forgetting
test's turned one, at block sizes 2, 4 and 8.  On every block the restatement is sure of, the kernel's flag must be its answer.
CPU only; needs the reference tree and says so where it is absent.  Run by tests/test_mapper_decay_host.py in a process of its own,
because the reference's package is called ``curobo`` like this repository's facade.
    python tests/mapper_decay_warp_check.py"""
import os
import sys

import numpy as np

REFERENCE = "/root/reference"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if not os.path.isdir(os.path.join(REFERENCE, "curobo", "_src", "perception", "mapper")):
    print("no reference tree here: nothing to compare; 0 failed")
    sys.exit(0)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
sys.path.insert(0, REFERENCE)
import make_scene_warp_golden as _emu  # noqa: E402,F401  (the Warp stand-in + module stubs)
import warp as wp  # noqa: E402
from curobo._src.perception.mapper.kernel.builder.builder_decay import make_decay_kernels  # noqa: E402

import mapper_cases as C  # noqa: E402
import mapper_decay_cases as DC  # noqa: E402
import mapper_decay_ref as DR  # noqa: E402

bad = compared = 0
for bs in DC.BLOCK_SIZES:
    g = DC.grid(bs)
    nbx, nby, nbz = g.nb
    b = np.arange(g.n_blocks)
    # the reference's block keys are centred: key = index - blocks // 2 (builder_decay.py:147-152)
    keys = np.stack([b % nbx - nbx // 2, (b // nbx) % nby - nby // 2, b // (nbx * nby) - nbz // 2], -1).astype(np.int32).reshape(-1)
    turned = DC.turned_frame()
    for name, (K, pos, quat), (dmin, dmax) in (("frustum test", DC.frustum_cameras(), DC.FRUSTUM_DEPTH),
                                               ("turned camera", turned[1:], (g.depth_min, g.depth_max))):
        kernels = make_decay_kernels(bs, grid_shape=(g.nz, g.ny, g.nx), origin_xyz=tuple(g.origin), voxel_size=g.vs, num_cameras=len(K),
                                     image_height=C.H, image_width=C.W, free_list_push=lambda *a: None)
        flags = np.zeros(g.n_blocks, np.int32)
        wp.launch(kernels["mark_blocks_in_frustum_kernel"], dim=(g.n_blocks, len(K)),
                  inputs=[wp.array(keys, dtype=wp.int32), wp.array(np.zeros(g.n_blocks, np.int32), dtype=wp.int32),
                          wp.array(np.array([g.n_blocks], np.int32), dtype=wp.int32), wp.array(np.asarray(K, np.float32), dtype=wp.float32),
                          wp.array(np.asarray(pos, np.float32), dtype=wp.float32), wp.array(np.asarray(quat, np.float32), dtype=wp.float32),
                          float(dmin), float(dmax), wp.array(flags, dtype=wp.int32), g.n_blocks])
        sure_in, sure_out = DR.frustum_flags(g, K, pos, quat, C.H, C.W, dmin, dmax)
        wrong = int((sure_in & (flags == 0)).sum() + (sure_out & (flags != 0)).sum())
        either = int((~sure_in & ~sure_out).sum())
        print(f"block size {bs}, {name}: {int((flags != 0).sum())} of {g.n_blocks} blocks flagged by the kernel, {int(sure_in.sum())} sure in, "
              f"{int(sure_out.sum())} sure out, {either} either, {wrong} disagree")
        bad += wrong
        compared += int(sure_in.sum() + sure_out.sum())
        assert sure_in.sum() >= 20 and sure_out.sum() >= 20 and either <= 0.01 * g.n_blocks
print(f"{compared} flags compared, {bad} failed")
sys.exit(1 if bad else 0)
