"""The record sort's geometry restated in Python from the rules the comments
of csrc/ctg_plan.h give (not from its loops), for tests/test_plan.py (against
tools/plan_check.cpp, no GPU) and tests/test_gpu_label_widths.py (against what
rag.last_sort() reports of a call).

Keys: a record's packed key is pk = (u << nb) | v with u < v, nb the bits of
the largest label.  The group sort puts pk into bucket (pk >> shift) - bk0,
bk0 the bucket of the smallest possible key."""

GS_M = 65536          # buckets at most
GS_TARGET = 3072      # records a bucket averages at most
GS_GB = 11            # group bits of the in-bucket counting sort
GS_CAP = 8192         # records a bucket holds at most (checked on the device counts, not by the plan)
BK_MAX_BITS = 12      # the packed-key bucket sort: 4096 buckets at most
SORT_WIDE_DIGITS_MAX = 64 << 20
BUCKET_PAIRS_MAX = 32 << 20

# ctg_last_sort's names (cluster_tools_amd/rag.py)
DECLINES = ('none', 'n_range', 'key_bits', 'item_bits', 'low_bits', 'bucket_cap')


def bits_for(v):
    return max(1, int(v).bit_length())


def key_range(nb, ub, min_label, max_label):
    """Smallest and largest packed key of edges (u, v), min_label <= u < v <=
    max_label, u clamped to its ub bits."""
    top = (1 << ub) - 1
    return min(min_label, max_label, top) << nb, (min(max_label, top) << nb) | max_label


def plan_group_sort(n, nb, ub, ib, min_label, max_label):
    """-> dict(why, shift, nbk, bk0).  Buckets of 2^shift packed keys from the
    smallest to the largest key: the largest shift at which the buckets average
    at most GS_TARGET records, but never so small a shift that there are more
    than GS_M buckets.  Declined (why != 'none') when n is not in [1, 2^32),
    the key has more than 63 bits, a bucket-local key and the slot do not fit
    one 64-bit item, or the bucket-local key below the GS_GB group bits does
    not fit 32 bits."""
    if not 0 < n < (1 << 32):
        return dict(why='n_range')
    kb = ub + nb
    if kb > 63:
        return dict(why='key_bits')
    lo, hi = key_range(nb, ub, min_label, max_label)

    def count(s):
        return (hi >> s) - (lo >> s) + 1
    # candidates from the widest buckets down: stop where the average fits or
    # where the next halving would pass GS_M buckets
    shift = next(s for s in range(kb, -1, -1) if s == 0 or count(s - 1) > GS_M or n <= GS_TARGET * count(s))
    out = dict(shift=shift, nbk=count(shift), bk0=lo >> shift, min_pk=lo, max_pk=hi)
    if shift + ib > 64:
        out['why'] = 'item_bits'
    elif shift - min(GS_GB, shift) > 32:
        out['why'] = 'low_bits'
    else:
        out['why'] = 'none'
    return out


def plan_bucket_keys(n, lo_bit, hi_bit, kmin, kmax):
    """The packed-key bucket sort: about 1 K keys a bucket (a power of two of
    buckets, 2 .. 4096, no more than the key has values), over [kmin, kmax]:
    the smallest shift >= lo_bit at which that many buckets still cover the
    range.  -> dict(ok, bb, shift, nbk, bk0)."""
    if not (0 < n < (1 << 32)) or hi_bit > 64 or lo_bit < 0 or hi_bit <= lo_bit or kmin > kmax:
        return dict(ok=0)
    bb = 1
    while bb < BK_MAX_BITS and n >= (1 << (bb + 10)):
        bb += 1
    bb = min(bb, hi_bit - lo_bit)

    def count(s):
        return (kmax >> s) - (kmin >> s) + 1
    shift = next((s for s in range(lo_bit, hi_bit - bb + 1) if count(s) <= (1 << bb)), hi_bit - bb)
    if count(shift) > (1 << BK_MAX_BITS):
        return dict(ok=0)
    return dict(ok=1, bb=bb, shift=shift, nbk=count(shift), bk0=kmin >> shift)


def plan_record_sort(n, ub, nb, ib, spread, has_keys=True, has_regions=True):
    """Default switches.  -> (packed, try_group, path): scan records pack their
    slot beside the key where ub + nb + ib <= 63 (and n is within the wide
    digits' range); records that do not pack are offered to the group sort
    when their top key bits are label bits (spread); otherwise bucket passes
    for spread keys and onesweep for tagged ones."""
    packed = has_keys and has_regions and ub + nb + ib <= 63 and n <= SORT_WIDE_DIGITS_MAX
    try_group = has_keys and has_regions and not packed and spread
    if packed:
        path = 'bucket_keys' if spread else 'onesweep_keys'
    elif spread and n <= BUCKET_PAIRS_MAX:
        path = 'bucket_pairs'
    else:
        path = 'onesweep_pairs_wide' if n <= SORT_WIDE_DIGITS_MAX else 'onesweep_pairs_default'
    return packed, try_group, path


def predict(info, min_label, max_label, spread=True):
    """What a call with default switches must have reported (rag.last_sort()),
    from its own ib, nb, ub and n and the labels of its edges (spread: a whole
    array; False for the block-tagged keys of a batched call): the fields
    path, packed, group_tried, group_decline (None where the decision needs
    the device's bucket counts: an accepted geometry)."""
    packed, try_group, path = plan_record_sort(info['n'], info['ub'], info['nb'], info['ib'], spread)
    exp = dict(packed=int(packed), group_tried=int(try_group), path=path, group_decline='none', plan=None)
    if try_group:
        g = plan_group_sort(info['n'], info['nb'], info['ub'], info['ib'], min_label, max_label)
        exp['plan'] = g
        exp['group_decline'] = g['why'] if g['why'] != 'none' else None
        if g['why'] == 'none':
            exp['path'] = None      # group sort, or the fallback where a bucket passes GS_CAP
            exp['packed'] = None
    return exp
