"""Scalar restatement of src/Encodings/splitbases.jl for the tests: plain Python floats and lists, loop for loop, one function per
reference function (line numbers in the docstrings), written independently of the vectorised code in mpstime.jl_amd/encodings.py
and used as its checker.  Indices are 0-based here; the 1-based counters of the reference (`i`, `j`) are kept where its
conditions are written in them.  Test infrastructure, like tests/analysis_ref.py."""
import math
import warnings
from fractions import Fraction


def get_nbins_safely(d, aux_basis_dim):
    """splitbases.jl:2-9."""
    if d % aux_basis_dim != 0:
        raise ValueError(f"The auxilliary basis dimension ({aux_basis_dim}) must evenly divide the total feature dimension ({d})")
    return int(d / aux_basis_dim)


def unif_split(nbins, a, b):
    """splitbases.jl:51-54, collect(a:dx:b): Julia lifts the end points of a float range to rationals, element i is the double
    nearest to a + i (b - a) / nbins, the last one is b."""
    return [float(Fraction(a) + i * (Fraction(b) - Fraction(a)) / nbins) for i in range(nbins + 1)]


def hist_split(samples, nbins, a, b):
    """splitbases.jl:56-88 for the samples of one time point."""
    samples = [float(s) for s in samples]
    npts = len(samples)
    bin_pts = int(round(npts / nbins))                 # Int(round(.)): half to even in both languages
    if bin_pts == 0:                                   # :60-63
        warnings.warn("Less than one data point per bin! Putting the extra bins at x=1 and hoping for the best")
        bin_pts = 1
    bins = [float(a)] * (nbins + 1)                    # :65
    j = 2                                              # :68 (1-based position of the next edge)
    ds = sorted(s for s in samples if a <= s <= b)     # :69
    for i, x in enumerate(ds, start=1):                # :70
        if i % bin_pts == 0 and i < len(samples):      # :71
            if j == nbins + 1:                         # :72-76
                break
            bins[j - 1] = (x + ds[i]) / 2              # :77, ds[i+1] (1-based); IndexError where Julia throws a BoundsError
            j += 1
    if j <= nbins:                                     # :81-84
        bins = [float(b) if e == a else e for e in bins]
        bins[0] = float(a)
    bins[-1] = float(b)                                # :86
    return bins


def hist_split_matrix(X_norm, nbins, a, b):
    """splitbases.jl:90-92; X_norm[i][t]: rows are series here, so a time point is a column."""
    T = len(X_norm[0])
    return [hist_split([row[t] for row in X_norm], nbins, a, b) for t in range(T)]


def rect(x, lbound=0.5, rbound=0.5):
    """splitbases.jl:96-108."""
    if x == -0.5:
        return lbound
    elif x == 0.5:
        return rbound
    elif -0.5 <= x <= 0.5:
        return 1.0
    else:
        return 0.0


def _div(num, den):
    """IEEE division as Julia's: x / 0 is +-Inf, 0 / 0 NaN"""
    if den == 0.0:
        return math.nan if (num == 0.0 or math.isnan(num)) else math.copysign(math.inf, num)
    return num / den


def project_onto_bins(x, aux_dim, aux_encoder, bins, norm=True):
    """splitbases.jl:113-132.  aux_encoder(xx, bin) returns the aux_dim coefficients (a list) of the auxiliary basis."""
    widths = [bins[i + 1] - bins[i] for i in range(len(bins) - 1)]
    a, b = bins[0], bins[-1]
    scale = b - a
    encoding = []
    for i, dx in enumerate(widths):
        y = 1.0 if norm else _div(1.0, dx)
        lbound = 1.0 if i == 0 else 0.5
        rbound = 1.0 if i == len(widths) - 1 else 0.5
        x_prop = _div(scale * (x - bins[i]), dx)
        select = y * rect(x_prop / scale - 0.5, lbound, rbound)
        if select == 0:
            encoding += [0.0] * aux_dim
        else:
            encoding += [select * v for v in aux_encoder(a + x_prop, i)]
    return encoding


def project_onto_bins_td(x, aux_dim, ti, aux_encoder, all_bins, norm=True):
    """splitbases.jl:144-163 for an auxiliary basis that is not time-dependent: site ti's edge list when there is one per site."""
    bins = all_bins[ti] if isinstance(all_bins[0], (list, tuple)) else all_bins
    return project_onto_bins(x, aux_dim, aux_encoder, bins, norm)
