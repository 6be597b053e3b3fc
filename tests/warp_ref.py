"""Float64 restatement of the affine warp family of csrc/warp.hip (F.affine_grid + F.grid_sample, align_corners=False) and
of the segmentation head fused with it.  No kernel logic: positions from the plain affine map, the eight trilinear corners
spelled out, the adjoint as an explicit scatter (index_add_) with no candidate search.  Licensed against torch's own
float64 grid_sample and autograd by tests/test_warp_ref.py; tests/test_gpu_warp.py measures the kernels against it.

Volumes are channels-last [B, D, H, W, C] float64; theta is [B, 3, 4] (rows x, y, z as at::affine_grid); sizes are
(D, H, W) tuples; pad is "zeros" or "border", interp "linear" or "nearest"."""
import torch


def base_coords(n):
    """Normalised coordinate of voxel j of n as at::affine_grid(align_corners=False) builds it: (2j + 1) / n - 1; 0 for n == 1."""
    if n == 1:
        return torch.zeros(1, dtype=torch.float64)
    return (2.0 * torch.arange(n, dtype=torch.float64) + 1.0) / n - 1.0


def sample_positions(theta, dst_size, src_size):
    """(ix, iy, iz), each [B, Dd, Hd, Wd] float64: the source-voxel position every destination voxel samples.
    g = theta . (x, y, z, 1) on the base coordinates of the destination, then i = ((g + 1) n - 1) / 2 on the source.
    The reference code builds its grid as (affine_grid(theta) - identity_grid) + identity_grid (`tta_grid_algebra`): in
    exact arithmetic that IS the plain affine map, so this restatement has one form for both."""
    th = theta.double()
    Dd, Hd, Wd = dst_size
    z = base_coords(Dd).view(1, Dd, 1, 1)
    y = base_coords(Hd).view(1, 1, Hd, 1)
    x = base_coords(Wd).view(1, 1, 1, Wd)
    out = []
    for row, n in zip(range(3), (src_size[2], src_size[1], src_size[0])):
        t = th[:, row].view(-1, 4, 1, 1, 1)
        g = t[:, 0] * x + t[:, 1] * y + t[:, 2] * z + t[:, 3]
        out.append(((g + 1.0) * n - 1.0) / 2.0)
    return tuple(out)


def _padded(pos, src_size, pad):
    if pad == "border":
        return tuple(p.clamp(0.0, float(n - 1)) for p, n in zip(pos, (src_size[2], src_size[1], src_size[0])))
    assert pad == "zeros"
    return pos


def _flat_index(cx, cy, cz, src_size):
    """(row index into [B * Vs], in-bounds mask) of lattice points (cx, cy, cz), each [B, ...] int64."""
    Ds, Hs, Ws = src_size
    inb = (cx >= 0) & (cx < Ws) & (cy >= 0) & (cy < Hs) & (cz >= 0) & (cz < Ds)
    b = torch.arange(cx.shape[0]).view(-1, 1, 1, 1)
    idx = ((b * Ds + cz.clamp(0, Ds - 1)) * Hs + cy.clamp(0, Hs - 1)) * Ws + cx.clamp(0, Ws - 1)
    return idx, inb


def _corners(pos):
    """The eight trilinear corners of every sample: (cx, cy, cz, weight)."""
    ix, iy, iz = pos
    fx, fy, fz = ix.floor(), iy.floor(), iz.floor()
    for k in range(8):
        dx, dy, dz = k & 1, (k >> 1) & 1, k >> 2
        wx = (ix - fx) if dx else (fx + 1.0 - ix)
        wy = (iy - fy) if dy else (fy + 1.0 - iy)
        wz = (iz - fz) if dz else (fz + 1.0 - iz)
        yield fx.long() + dx, fy.long() + dy, fz.long() + dz, wx * wy * wz


def warp(x, theta, dst_size, pad="zeros", interp="linear", sub=0.0):
    """dst[b, v] = sum over the in-volume corners of w (x[corner] - sub), + sub: grid_sample of x with the volume continued
    by `sub` outside (zeros padding) or by its faces (border padding).  Nearest: the voxel at the position rounded half to even."""
    B, Ds, Hs, Ws, C = x.shape
    src_size = (Ds, Hs, Ws)
    pos = _padded(sample_positions(theta, dst_size, src_size), src_size, pad)
    rows = (x.double() - sub).reshape(-1, C)
    if interp == "nearest":
        idx, inb = _flat_index(*(p.round().long() for p in pos), src_size)
        return rows[idx] * inb[..., None] + sub
    assert interp == "linear"
    out = torch.zeros(B, *dst_size, C, dtype=torch.float64)
    for cx, cy, cz, w in _corners(pos):
        idx, inb = _flat_index(cx, cy, cz, src_size)
        out += (w * inb)[..., None] * rows[idx]
    return out + sub


def warp_adjoint(g, theta, src_size, pad="zeros"):
    """Adjoint of the linear warp w.r.t. its source: every destination voxel adds w g to each of its in-volume corners."""
    B, Dd, Hd, Wd, C = g.shape
    pos = _padded(sample_positions(theta, (Dd, Hd, Wd), src_size), src_size, pad)
    out = torch.zeros(B * src_size[0] * src_size[1] * src_size[2], C, dtype=torch.float64)
    g = g.double()
    for cx, cy, cz, w in _corners(pos):
        idx, inb = _flat_index(cx, cy, cz, src_size)
        out.index_add_(0, idx[inb], (w[..., None] * g)[inb])
    return out.view(B, *src_size, C)


def warp_abs_adjoint(g, theta, src_size, pad="zeros"):
    """sum |w g| per source element (the weights are >= 0): what error bounds of the adjoint are proportional to."""
    return warp_adjoint(g.abs(), theta, src_size, pad)


def candidate_sums(g, theta, src_size, pad="zeros", tol=0.0):
    """(count, sum |g|) per source voxel / element over the destination voxels that can touch it: those whose sample has the
    voxel among its eight corners, and those whose position is within `tol` (per axis, in voxels) of having it - the samples
    for which arithmetic of that accuracy may floor to the neighbouring cell.  tol: a number, or one per axis (x, y, z), each
    a number or a tensor [B, 1, 1, 1].  count [B, Ds, Hs, Ws], sums [B, Ds, Hs, Ws, C]."""
    B, Dd, Hd, Wd, C = g.shape
    pos = _padded(sample_positions(theta, (Dd, Hd, Wd), src_size), src_size, pad)
    if not isinstance(tol, (tuple, list)):
        tol = (tol, tol, tol)
    nrow = B * src_size[0] * src_size[1] * src_size[2]
    cnt = torch.zeros(nrow, dtype=torch.float64)
    sums = torch.zeros(nrow, C, dtype=torch.float64)
    ga = g.double().abs()
    axes = []
    for p, t in zip(pos, tol):
        f = p.floor()
        fr = p - f
        one = torch.ones_like(fr, dtype=torch.bool)
        axes.append([(f.long() + o, m) for o, m in ((-1, fr <= t), (0, one), (1, one), (2, fr >= 1.0 - t))])
    for cx, mx in axes[0]:
        for cy, my in axes[1]:
            for cz, mz in axes[2]:
                idx, inb = _flat_index(cx, cy, cz, src_size)
                m = inb & mx & my & mz
                if bool(m.any()):
                    cnt.index_add_(0, idx[m], torch.ones(int(m.sum()), dtype=torch.float64))
                    sums.index_add_(0, idx[m], ga[m])
    return cnt.view(B, *src_size), sums.view(B, *src_size, C)


def head(z, w, bias, sel=None):
    """The 1x1x1 segmentation head on the selected rows: z [B, D, H, W, Cin] -> [B, D, H, W, nsel]."""
    if sel is not None:
        w, bias = w[sel], bias[sel]
    return z.double() @ w.double().t() + bias.double()


def head_then_warp(z, w, bias, sel, theta):
    """warp(z W^T + b) with zeros padding onto the lattice of z."""
    return warp(head(z, w, bias, sel), theta, tuple(z.shape[1:4]), "zeros", "linear")


def head_then_warp_grads(z, w, sel, theta, gout):
    """Gradients of sum(head_then_warp * gout): (gl, gz, dw_sel, db_sel) with gl the gradient of the un-warped logits
    (the adjoint above), gz = gl W_sel, dw_sel[k][c] = sum_v gl[v][k] z[v][c], db_sel[k] = sum_v gl[v][k]."""
    ws = (w if sel is None else w[sel]).double()
    gl = warp_adjoint(gout, theta, tuple(z.shape[1:4]), "zeros")
    gz = gl @ ws
    dw = torch.einsum("bdhwk,bdhwc->kc", gl, z.double())
    db = gl.sum(dim=(0, 1, 2, 3))
    return gl, gz, dw, db
