"""How much of what a tile's backward walks can reach the tile at all? CPU statistics from the oracle's lists (no GPU).

    python tools/list_liveness.py [P = 3000000] [scale_sigma = 0.6]        (run from the repository root)

For a synth-v1 view (1920x1080, indexed) it restates in numpy the forward's exact-conservative quadrant test (`quadrant_mask`,
csrc/render.hip) and the backward's per-wave depth cut on the oracle's sorted lists, and counts ENTRIES, not (wave, entry) pairs:
  * entries a tile visits (the prefix up to its deepest last contributor), and the share whose mask is 0 -- they reach no pixel
    of the tile, and the forward leaves them out of the compact list the backward walks;
  * (wave, entry) pairs the backward blends (the figure tools/lane_efficiency.py measures on the device) and entries no wave lists;
  * rounds of 256 the backward runs over list positions vs over live entries only;
  * Gaussians with a visited / a live instance (the latter reach backward_preprocess);
  * a float64 check that every dropped entry has alpha < 1/255 at all 256 pixels of its tile.
"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.getcwd())
from oracle import oracle as orc  # noqa: E402
from tests import synth  # noqa: E402

f32 = np.float32


def quadrant_masks(mx, my, ca, cb, cc, op, tx0, ty0):
    """numpy restatement of quadrant_mask() of csrc/render.hip (float32 throughout). -> int64 mask per entry, bit q = qy*2+qx"""
    with np.errstate(all="ignore"):
        tau = np.log(f32(255.0) * op).astype(f32) * f32(1.0001) + f32(1e-4)
        det = ca * cc - cb * cb
        nocull = ~(det > 0) | ~(ca > 0) | ~(cc > 0) | ~(tau < 1e30)
        nb_c, nb_a = -cb / cc, -cb / ca

        def fq(dx, dy):
            return f32(0.5) * (ca * dx * dx + cc * dy * dy) + cb * dx * dy

        mask = np.zeros(len(mx), np.int64)
        for q in range(4):
            x0 = tx0 + f32((q & 1) * 8) - f32(0.01) - mx
            y0 = ty0 + f32((q >> 1) * 8) - f32(0.01) - my
            x1, y1 = x0 + f32(7.02), y0 + f32(7.02)
            inside = (x0 <= 0) & (x1 >= 0) & (y0 <= 0) & (y1 >= 0)
            ya = np.minimum(np.maximum(nb_c * x0, y0), y1)
            yb = np.minimum(np.maximum(nb_c * x1, y0), y1)
            xa = np.minimum(np.maximum(nb_a * y0, x0), x1)
            xb = np.minimum(np.maximum(nb_a * y1, x0), x1)
            fmin = np.minimum(np.minimum(fq(x0, ya), fq(x1, yb)), np.minimum(fq(xa, y0), fq(xb, y1)))
            fmin = np.where(inside, f32(0), fmin)
            mask |= (~(fmin > tau)).astype(np.int64) << q
        mask = np.where(nocull, 15, mask)
        return np.where(op < f32(1.0 / 255.0) * f32(0.999), 0, mask)


def main():
    P = int(sys.argv[1]) if len(sys.argv) > 1 else 3_000_000
    sigma = float(sys.argv[2]) if len(sys.argv) > 2 else 0.6
    W, H, focal = 1920, 1080, 1200.0
    intr, ev = synth.camera(W, H, focal)
    ix = synth.index_scene(synth.scene(P, W, H, focal, seed=1234, sh_degree=3, scale_sigma=sigma))
    cam = orc.camera(intr.numpy(), ev.numpy())
    t0 = time.time()
    st = orc.rasterize_forward(bg=np.zeros(3, np.float32), means3D=ix["means3D"].numpy(), opacities=ix["opacities"].numpy(),
                               shs=ix["shs"].numpy(), scales=ix["scales"].numpy(), rotations=ix["rotations"].numpy(),
                               scale_factors=ix["scale_factors"].numpy(), sh_indices=ix["sh_indices"].numpy(),
                               g_indices=ix["g_indices"].numpy(), degree=3, clamp_color=True, **cam)
    print(f"P={P} scale_sigma={sigma}: oracle forward {time.time() - t0:.1f} s, R={st.num_rendered}", flush=True)
    gx, gy = (W + 15) // 16, (H + 15) // 16
    T = gx * gy
    pad = np.zeros((gy * 16, gx * 16), np.int64)
    pad[:H, :W] = st.n_contrib.reshape(H, W)
    tile_used = pad.reshape(gy, 16, gx, 16).max(axis=(1, 3)).reshape(-1)
    wave_last = pad.reshape(gy, 2, 8, gx, 2, 8).max(axis=(2, 5)).transpose(0, 2, 1, 3).reshape(T, 4)   # per quadrant q = qy*2+qx
    rg = st.ranges.astype(np.int64)
    n = rg[:, 1] - rg[:, 0]
    used = np.minimum(n, tile_used)
    E = int(used.sum())
    print(f"visited entries {E} of {int(n.sum())} listed ({E / max(int(n.sum()), 1):.3f})")
    tiles = np.repeat(np.arange(T), used)
    pos = np.arange(E) - np.repeat(np.cumsum(used) - used, used)
    ids = st.point_list[rg[tiles, 0] + pos]
    m, co = st.means2D[ids].astype(f32), st.conic_opacity[ids].astype(f32)
    mx, my, ca, cb, cc, op = m[:, 0], m[:, 1], co[:, 0], co[:, 1], co[:, 2], co[:, 3]
    tx0, ty0 = ((tiles % gx) * 16).astype(f32), ((tiles // gx) * 16).astype(f32)
    mask = quadrant_masks(mx, my, ca, cb, cc, op, tx0, ty0)
    bits = np.array([bin(i).count("1") for i in range(16)])
    print(f"mask == 0 (no quadrant): {(mask == 0).mean():.3f} of the visited entries; quadrants per entry {bits[mask].mean():.3f}")
    # backward: wave q lists an entry iff bit q is set and the entry lies in front of the wave's deepest last contributor
    bw = np.zeros(E, np.int64)
    for q in range(4):
        bw |= (((mask >> q) & 1).astype(bool) & (pos < wave_last[tiles, q])).astype(np.int64) << q
    print(f"backward (wave, entry) pairs {int(bits[bw].sum())}; entries no backward wave lists {(bw == 0).mean():.3f}")
    live_per_tile = np.bincount(tiles, weights=(mask != 0), minlength=T).astype(np.int64)
    r_now, r_live = int(((used + 255) // 256).sum()), int(((live_per_tile + 255) // 256).sum())
    print(f"backward rounds of 256: over positions {r_now}, over live entries {r_live} ({r_live / max(r_now, 1):.2f}x)")
    print(f"Gaussians with a visited instance {np.unique(ids).size}, with a live instance {np.unique(ids[mask != 0]).size}, "
          f"visible {int((st.radii > 0).sum())}")
    # float64: a dropped entry blends nowhere in its tile
    dead = np.nonzero(mask == 0)[0]
    ox, oy = np.meshgrid(np.arange(16.0), np.arange(16.0))
    ox, oy = ox.reshape(1, -1), oy.reshape(1, -1)
    worst, bad = 0.0, 0
    for s0 in range(0, len(dead), 100_000):
        d = dead[s0:s0 + 100_000]
        dx = mx[d].astype(np.float64)[:, None] - (tx0[d].astype(np.float64)[:, None] + ox)
        dy = my[d].astype(np.float64)[:, None] - (ty0[d].astype(np.float64)[:, None] + oy)
        pw = (-0.5 * (ca[d].astype(np.float64)[:, None] * dx * dx + cc[d].astype(np.float64)[:, None] * dy * dy)
              - cb[d].astype(np.float64)[:, None] * dx * dy)
        al = np.where(pw > 0, 0.0, op[d].astype(np.float64)[:, None] * np.exp(np.minimum(pw, 0.0)))
        worst = max(worst, float(al.max()))
        bad += int((al >= 1.0 / 255.0).sum())
    print(f"dropped entries {len(dead)}: largest alpha x 255 over their tiles {worst * 255.0:.4f}, (pixel, entry) pairs at or above 1/255: {bad}")


if __name__ == "__main__":
    main()
