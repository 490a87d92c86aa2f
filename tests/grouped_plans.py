"""Routing-plan builders shared by the grouped (MoE) GEMM tests: a tile -> expert table with holes and the inverse map of a top-2
routing (sorted position -> token row, -1 = padding) with ragged segment fills.  Plain torch on the CPU; the draws come from the
caller's generator in a fixed order, so a test's seed names its plan."""
import torch


def expert_table(E, ntile, holes, gen):
    """expert of each 256-row tile, drawn uniformly; the tiles listed in `holes` are padding segments (-1)"""
    te = torch.randint(0, E, (ntile,), generator=gen).tolist()
    for hole in holes:
        te[hole] = -1
    return te


def ragged_row_map(te, T, gen):
    """int32 [256 * len(te)]: every one of T tokens twice (two permutations back to back), dealt to the real tiles in order; every third
    tile is full, the others end in 1 ... 71 padding rows (-1); padding segments hold -1 throughout"""
    row_map = torch.full((256 * len(te),), -1, dtype=torch.int32)
    src = torch.cat([torch.randperm(T, generator=gen), torch.randperm(T, generator=gen)]).to(torch.int32)
    cursor = 0
    for t_, ex in enumerate(te):
        if ex < 0:
            continue
        cnt = 256 if t_ % 3 else 256 - 7 * (t_ % 11) - 1  # ragged fill: padding rows behind the entries of some real tiles
        cnt = min(cnt, src.numel() - cursor)
        row_map[256 * t_: 256 * t_ + cnt] = src[cursor:cursor + cnt]
        cursor += cnt
    return row_map


def filled_row_map(ntile, fill, T, gen):
    """int32 [256 * ntile] with fill[t] entries at the head of tile t, taken in order from one permutation of the T tokens written twice;
    returns (row_map, entries dealt)"""
    row_map = torch.full((256 * ntile,), -1, dtype=torch.int32)
    perm = torch.randperm(T, generator=gen)
    cursor = 0
    for t_, cnt in fill.items():
        idx = torch.cat([perm, perm])[cursor:cursor + cnt]
        cursor += cnt
        row_map[256 * t_: 256 * t_ + cnt] = idx.to(torch.int32)
    return row_map, cursor


def gather_rows(X, row_map):
    """[len(row_map), K] copy of the rows row_map names, zeros where it says -1 (plain indexing: what gather-on-load must read)"""
    rm = row_map.to(X.device).long()
    out = X[rm.clamp_min(0)].clone()
    out[rm < 0] = 0
    return out
