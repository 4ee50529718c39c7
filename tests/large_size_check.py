"""Maximum-size checks, run as a separate process by tests/test_gpu_large.py (torch is used to
build multi-GB device inputs and has to be imported before libc2d.so).

  1. 1.2e9 rectangle pairs: every plane is 4.8 GB, so element offsets pass 2^32 bytes and the
     launch has 4.7e6 blocks.  The input is a 2e6-pair block repeated 600 times; the output must
     be 600 copies of the oracle's booleans for that block and the count 600 x the block's count.
     The same planes through c2d_sat_rect_pairs_verts_mask: the 150 MB bit mask must be 600 copies of the block's bits.
  2. c2d_sat_rect_pairs_aos over 1.4e8 + 1 pairs: each f32[n][8] rectangle array is 4.5 GB, so rectangle offsets pass 2^32 bytes.
  3. Monte-Carlo sample indices beyond 2^32: hits over [2^32 - 1e6, 2^32 + 1e6) must equal the
     oracle's, and a 6e9-sample range must equal the sum of its two halves.
TEST INFRASTRUCTURE: uses the oracle as the checker."""
import os
import sys

import torch
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from __graft_entry__ import load_package  # noqa: E402

pkg = load_package()
import importlib  # noqa: E402

wl = importlib.import_module("c2d_amd.workloads")
from oracle import cpu as oracle  # noqa: E402


def main():
    eng = pkg.Engine(0)
    dev = torch.device("cuda", 0)
    B, R = 2_000_000, 600
    n = B * R
    poses = wl.random_obb_pose_planes(B, seed=77, extent=4.0)
    block = np.concatenate([oracle.rects_from_poses(*poses[:5]), oracle.rects_from_poses(*poses[5:])])
    ref, ref_cnt = oracle.sat_rect_pairs_verts(block)
    blk = torch.from_numpy(block).to(dev)
    planes = torch.empty((16, n), dtype=torch.float32, device=dev)
    planes.view(16, R, B)[:] = blk[:, None, :]
    out = torch.empty(n, dtype=torch.uint8, device=dev)
    cnt = torch.zeros(1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    row = lambda t, k: t.data_ptr() + k * t.stride(0) * t.element_size()  # noqa: E731
    eng.sat_rect_pairs_verts([row(planes, k) for k in range(16)], n, out.data_ptr(), cnt.data_ptr())
    torch.cuda.synchronize()
    assert int(cnt.item()) == R * ref_cnt, (int(cnt.item()), R * ref_cnt)
    refd = torch.from_numpy(ref).to(dev)
    assert bool((out.view(R, B) == refd[None, :]).all()), "booleans differ somewhere in the 1.2e9-pair batch"
    print(f"large SAT ok: {n} pairs, plane size {4 * n / 1e9:.1f} GB, count {int(cnt.item())}")
    del out
    words = n // 64
    assert words * 64 == n and B % 64 == 0
    mask = torch.full((words + 1,), -1, dtype=torch.int64, device=dev)   # poisoned, one word past the end that must stay so
    cnt.zero_()
    eng.sat_rect_pairs_verts_mask([row(planes, k) for k in range(16)], n, mask.data_ptr(), cnt.data_ptr())
    torch.cuda.synchronize()
    assert int(cnt.item()) == R * ref_cnt, (int(cnt.item()), R * ref_cnt)
    ref_bits = torch.from_numpy(np.packbits(ref, bitorder="little")).to(dev)   # (little-endian bits in little-endian words)
    assert bool((mask[:words].view(torch.uint8).view(R, B // 8) == ref_bits[None, :]).all()), "mask bits differ somewhere in the 1.2e9-pair batch"
    assert int(mask[words].item()) == -1, "the mask was written past its last word"
    print(f"large SAT mask ok: {n} pairs, {8 * words / 1e6:.0f} MB of mask")
    del planes, mask
    torch.cuda.empty_cache()

    n_aos = 140_000_001
    R_aos, tail = divmod(n_aos, B)
    assert 32 * n_aos > 2**32
    out = torch.full((n_aos,), 7, dtype=torch.uint8, device=dev)
    rects = []
    for half in (blk[:8], blk[8:]):   # rectangle i of a side = its 8 vertex coordinates, f32[n][8]
        aos = torch.empty((n_aos, 8), dtype=torch.float32, device=dev)
        aos[:R_aos * B].view(R_aos, B, 8).copy_(half.t()[None].expand(R_aos, B, 8))
        aos[R_aos * B:] = half.t()[:tail]
        rects.append(aos)
    cnt.zero_()
    torch.cuda.synchronize()
    eng.sat_rect_pairs_aos(rects[0].data_ptr(), rects[1].data_ptr(), n_aos, out.data_ptr(), cnt.data_ptr())
    torch.cuda.synchronize()
    assert bool((out[:R_aos * B].view(R_aos, B) == refd[None, :]).all()) and bool((out[R_aos * B:] == refd[:tail]).all()), "AoS booleans differ"
    want = R_aos * ref_cnt + int(ref[:tail].sum())
    assert int(cnt.item()) == want, (int(cnt.item()), want)
    print(f"large AoS ok: {n_aos} pairs, rectangle arrays of {32 * n_aos / 1e9:.1f} GB")
    del rects, out
    torch.cuda.empty_cache()

    sc = wl.MC_PAIR_SCENE
    args = (sc["robot_w"], sc["robot_h"], sc["pos"], sc["pose"], sc["std_dev"], 99, 7)
    hits = torch.zeros(1, dtype=torch.int64, device=dev)

    def gpu(begin, count):
        hits.zero_()
        eng.mc_pair(*args, begin, count, hits.data_ptr())
        torch.cuda.synchronize()
        return int(hits.item())

    b0 = (1 << 32) - 1_000_000
    assert gpu(b0, 2_000_000) == oracle.mc_pair(*args, b0, 2_000_000)
    whole = gpu(0, 6_000_000_000)
    assert whole == gpu(0, 3_000_000_001) + gpu(3_000_000_001, 2_999_999_999)
    print(f"large MC ok: 6e9 samples, p = {whole / 6e9:.6f}")


if __name__ == "__main__":
    main()
    print("large size ok")
