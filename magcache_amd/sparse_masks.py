"""Block masks for the tile-sparse self-attention (Engine.set_attention_tile_mask, mc_op_attention_sparse), built on the CPU.

A mask is a bool tensor [mask_heads, nqt, nkt] over (128-row query tile, 64-key tile) of the token sequence padded to
Lp = a multiple of 256 rows: nqt = Lp / 128, nkt = Lp / 64.  The kernel is tile-granular by contract, so a rule stated on
elements is served by its conservative TILE COVER: tile (qt, kt) is visible iff some visible element pair (i, j), i, j < L,
lies inside it.  Nothing here loops over elements at real sizes: temporal_decay_tile_mask works on (query tile, key frame)
intervals.

The MM-DiT engine (MMDiTEngine.set_attention_tile_mask, mc_op_attention_joint_sparse) takes the same words over its JOINT text +
image rows; joint_tile_mask lifts an image mask there and leaves the text bits clear, because that kernel supplies the text rule."""
import numpy as np
import torch

QT, KT = 128, 64     # query rows and keys per tile of attention_sparse.hip


def padded_len(L):
    """the engine's Lp: L padded to whole 256-row query blocks"""
    return (int(L) + 255) // 256 * 256


def pack_tile_mask(mask):
    """bool [mask_heads, nqt, nkt] -> int32 [mask_heads, nqt, (nkt + 31) / 32], contiguous, on the CPU: key tile kt is bit
    kt & 31 of word kt >> 5 (the uint32 words of mc_op_attention_sparse, carried as int32)"""
    m = torch.as_tensor(mask).detach().cpu().numpy().astype(bool)
    mh, nqt, nkt = m.shape
    words = (nkt + 31) // 32
    padded = np.zeros((mh, nqt, words * 32), dtype=bool)
    padded[:, :, :nkt] = m
    bits = np.packbits(padded.reshape(mh, nqt, words, 32), axis=-1, bitorder="little")          # 4 bytes per word, low first
    return torch.from_numpy(np.ascontiguousarray(bits).view("<u4").reshape(mh, nqt, words).view(np.int32).copy())


def unpack_tile_mask(words, nkt):
    """the inverse of pack_tile_mask: int32 [mask_heads, nqt, words] -> bool [mask_heads, nqt, nkt]"""
    w = np.ascontiguousarray(torch.as_tensor(words).cpu().numpy().view(np.uint32)).astype("<u4")
    bits = np.unpackbits(w.view(np.uint8).reshape(w.shape + (4,)), axis=-1, bitorder="little")
    return torch.from_numpy(bits.reshape(w.shape[0], w.shape[1], -1)[:, :, :nkt].astype(bool))


def tile_cover(vis, L):
    """The conservative tile cover of an element rule over L tokens -> bool [Lp / 128, Lp / 64].  vis: a bool [L, L] element
    mask (numpy or torch), or a callable vis(i, j) -> bool array over broadcast index arrays.  The callable form evaluates
    128 query rows at a time: L x 128 elements in flight, for checking a builder at small L, not for real sizes."""
    L = int(L)
    Lp = padded_len(L)
    nqt, nkt = Lp // QT, Lp // KT
    out = np.zeros((nqt, nkt), dtype=bool)
    j = np.arange(L)
    for qt in range((L + QT - 1) // QT):
        i = np.arange(qt * QT, min((qt + 1) * QT, L))
        rows = vis(i[:, None], j[None, :]) if callable(vis) else np.asarray(torch.as_tensor(vis)[i[0]:i[-1] + 1].cpu().numpy())
        cols = np.zeros(nkt * KT, dtype=bool)
        cols[:L] = np.asarray(rows, dtype=bool).any(0)
        out[qt] = cols.reshape(nkt, KT).any(1)
    return torch.from_numpy(out)


def shard_tile_cover(vis, L, rank, P):
    """tile_cover in the tile space of a sequence-parallel engine (Engine.set_sharded_attention_tile_mask): rank p holds the
    tokens [p Lr, (p + 1) Lr), Lr = L / P, as rows 0 .. Lr - 1 of a shard padded to Lp = padded_len(Lr).  Returns bool
    [Lp / 128, P * Lp / 64] for `rank`: row qt = this rank's query tile qt, column p * (Lp / 64) + t = key tile t of rank p's shard
    -- tiles are counted per shard, because Lr need not be a multiple of 64.  vis as in tile_cover (indices are global
    tokens); like tile_cover, for small sizes.  P = 1 is tile_cover."""
    L, rank, P = int(L), int(rank), int(P)
    if P < 1 or L % P or not 0 <= rank < P:
        raise ValueError(f"shard_tile_cover: L {L} must divide into P {P} shards and rank {rank} lie in [0, P)")
    Lr = L // P
    Lp = padded_len(Lr)
    nqt, tpr = Lp // QT, Lp // KT
    out = np.zeros((nqt, P * tpr), dtype=bool)
    j = np.arange(L)
    for qt in range((Lr + QT - 1) // QT):
        i = rank * Lr + np.arange(qt * QT, min((qt + 1) * QT, Lr))
        rows = vis(i[:, None], j[None, :]) if callable(vis) else np.asarray(torch.as_tensor(vis)[i[0]:i[-1] + 1].cpu().numpy())
        cols = np.zeros((P, tpr * KT), dtype=bool)
        cols[:, :Lr] = np.asarray(rows, dtype=bool).any(0).reshape(P, Lr)
        out[qt] = cols.reshape(P * tpr, KT).any(1)
    return torch.from_numpy(out)


def joint_tile_mask(image_mask, text_first, txt_len, img_tokens):
    """Lift a mask over the IMAGE tokens to the joint rows of an MM-DiT engine (MMDiTEngine.set_attention_tile_mask).
    image_mask: bool [mask_heads, >= ceil(Li / 128), >= ceil(Li / 64)] over tiles of the Li = img_tokens image tokens counted
    from 0 (what a grid builder such as temporal_decay_tile_mask returns); the joint rows are [text ; image] (text_first: FLUX,
    Qwen-Image) or [image ; text] (HunyuanVideo), S = txt_len + Li of them, padded to Sp.  Element rule: joint rows (i, j) that
    are both image rows are visible iff image_mask holds tile ((i - img0) / 128, (j - img0) / 64), img0 = the first image row;
    a pair with a text row is NOT stated here -- the kernel supplies the text rule (every query sees the valid text keys, text
    queries see everything), so text bits stay clear.  Returns the tile cover of that rule, bool [mask_heads, Sp / 128,
    Sp / 64]: the image tiles offset by img0, which need not be a multiple of the tile (a joint tile then covers two image
    tiles and takes the union)."""
    m = torch.as_tensor(image_mask).detach().cpu().numpy().astype(bool)
    Lt, Li = int(txt_len), int(img_tokens)
    if m.ndim != 3 or m.shape[1] < (Li + QT - 1) // QT or m.shape[2] < (Li + KT - 1) // KT:
        raise ValueError(f"joint_tile_mask: a bool [mask_heads, >= {(Li + QT - 1) // QT}, >= {(Li + KT - 1) // KT}] image mask, got {m.shape}")
    img0 = Lt if text_first else 0
    Sp = padded_len(Lt + Li)

    def spans(tile, n):   # per joint tile: does it hold image rows, and the first and last image tile they fall into
        t = np.arange(n)
        lo = np.maximum(t * tile, img0) - img0
        hi = np.minimum((t + 1) * tile, img0 + Li) - 1 - img0
        ok = hi >= lo
        return ok, np.where(ok, lo // tile, 0), np.where(ok, hi // tile, 0)
    okq, q_lo, q_hi = spans(QT, Sp // QT)
    okk, k_lo, k_hi = spans(KT, Sp // KT)
    out = np.zeros((m.shape[0], Sp // QT, Sp // KT), dtype=bool)
    for qa in (q_lo, q_hi):
        for ka in (k_lo, k_hi):
            out |= m[:, qa][:, :, ka]
    return torch.from_numpy(out & okq[None, :, None] & okk[None, None, :])


def decay_shift(d, dense_frames):
    """s = floor(log2(d / dense_frames)) + 1 for integer frame distances d >= dense_frames, in integers"""
    d = np.asarray(d, dtype=np.int64)
    s = np.zeros_like(d)
    while True:
        more = (dense_frames << s) <= d
        if not more.any():
            return s
        s = s + more


def temporal_decay_tile_mask(grid, dense_frames=1, sink_frames=1):
    """Temporal-decay attention in the spirit of radial attention, stated as this project's own rule.  Tokens are frame-major
    over the latent grid (F, H, W): tpf = (H / 2)(W / 2) tokens per frame, token i lies in frame fi = i // tpf at position
    i % tpf, d = |fi - fj|.  Pair (i, j) is visible iff
        d < dense_frames,  or  fj < sink_frames,  or  |i % tpf - j % tpf| * 2^s < tpf  with  s = floor(log2(d / dense_frames)) + 1:
    near frames whole, the first frames always, and a spatial window that halves each time the frame distance doubles.
    Returns the tile cover of that rule, bool [1, Lp / 128, Lp / 64]; query tiles that hold only padding rows see nothing
    (the kernel writes zeros there, nothing reads them)."""
    F, H, W = (int(v) for v in grid)
    dense_frames, sink_frames = int(dense_frames), int(sink_frames)
    if dense_frames < 1 or sink_frames < 0:
        raise ValueError(f"temporal_decay_tile_mask: dense_frames {dense_frames} must be >= 1 and sink_frames {sink_frames} >= 0")
    tpf = (H // 2) * (W // 2)
    L = F * tpf
    Lp = padded_len(L)
    nqt, nkt = Lp // QT, Lp // KT
    # segments: the rows of one query tile that lie in one frame, as positions [a, b] inside that frame
    q0 = np.arange((L + QT - 1) // QT) * QT
    q1 = np.minimum(q0 + QT, L) - 1
    f0, f1 = q0 // tpf, q1 // tpf
    n_seg = f1 - f0 + 1
    seg_qt = np.repeat(np.arange(len(q0)), n_seg)
    seg_f = np.concatenate([np.arange(a, b + 1) for a, b in zip(f0, f1)])
    a = np.maximum(q0[seg_qt], seg_f * tpf) - seg_f * tpf
    b = np.minimum(q1[seg_qt], seg_f * tpf + tpf - 1) - seg_f * tpf
    # per (segment, key frame): the visible positions of the key frame are ONE interval, the union of [p - w, p + w], p in [a, b]
    fj = np.arange(F)[None, :]
    d = np.abs(seg_f[:, None] - fj)
    whole = (d < dense_frames) | (fj < sink_frames)
    s = decay_shift(np.maximum(d, dense_frames), dense_frames)
    w = (tpf + (1 << s) - 1) // (1 << s) - 1                       # the largest distance with dist * 2^s < tpf
    lo = np.where(whole, 0, np.maximum(a[:, None] - w, 0)) + fj * tpf
    hi = np.where(whole, tpf - 1, np.minimum(b[:, None] + w, tpf - 1)) + fj * tpf
    # key tiles lo // 64 .. hi // 64 of the segment's query tile: +1 / -1 marks, one running sum per mask row
    marks = np.zeros((nqt, nkt + 1), dtype=np.int64)
    rows = np.broadcast_to(seg_qt[:, None], lo.shape)
    np.add.at(marks, (rows, lo // KT), 1)
    np.add.at(marks, (rows, hi // KT + 1), -1)
    return torch.from_numpy(np.cumsum(marks, axis=1)[:, :nkt] > 0)[None]
