# make_kde_goldens.jl - pins the Sahand-Legendre encodings of this repository (DESIGN.md, "Sahand-Legendre encodings") against
# KernelDensity.jl and the Julia reference.  The build image has no Julia, so this script has never been executed: it is written
# against the reference's source (file:line below) for a maintainer who has MPSTime.jl checked out.  Needs MPSTime, KernelDensity, NPZ.
#
#   julia --project=<MPSTime.jl checkout> tests/golden/make_kde_goldens.jl <repo>/tests/golden
#
# It builds a small deterministic training matrix (no random stream: the values are a closed formula, and they are stored with the
# results, so the Python side reads the very same doubles), then writes tests/golden/juliaref_kde.npz with
#   X (N, T), Xq (Nq, T), d                                 the training matrix, the query matrix, the basis dimension
#   bandwidth (T), grid_lo (T), grid_step (T), density (T, K)  KernelDensity.jl's estimate of every column: kde(xs) (default_bandwidth,
#                                                              the 2048-point grid, the binned and smoothed values)
#   pdf_q (Nq, T)                                           pdf(kde_t, Xq[:, t]): the quadratic B-spline interpolant, 0 outside the grid
#   minxs (T), scales (T), cvecs (T, d, d)                  init_sahand_legendre_time_dependent (src/Encodings/bases.jl:310-342)
#   phi_q (Nq, T, d)                                        sahand_legendre_encode (bases.jl:111-129) of every query value
#   ti_minx, ti_scale, ti_cvecs (d, d)                      the time-independent form with the sample points from a to b - the
#                                                           reference's own init samples range(-a, b, S), a constant vector for
#                                                           (-1, 1), so remove_zeros! and sahand_legendre_coeffs (bases.jl:158-206,
#                                                           :269-291) are called here on range(a, b, S) directly
# No test reads the file yet: the one that compares mpstime_jl_amd.encodings with it is added in the commit that adds the file.
using MPSTime, KernelDensity, NPZ
import MPSTime: init_sahand_legendre_time_dependent, sahand_legendre_encode, sahand_legendre_coeffs, remove_zeros!, safe_options

dir = ARGS[1]
N, T, Nq, d = 60, 4, 25, 4
X = [clamp(0.55 * sin(1.7 * i + 0.9 * t) + 0.35 * cos(0.37 * i * t) + 0.1, -1.0, 1.0) for i in 1:N, t in 1:T]
Xq = [clamp(0.9 * sin(0.61 * i + 1.3 * t), -1.0, 1.0) for i in 1:Nq, t in 1:T]
opts = safe_options(MPSOptions(; d=d, encoding=:SLTD, verbosity=-1, log_level=0))

# the density estimates themselves
kdes = [kde(X[:, t]) for t in 1:T]
K = length(kdes[1].x)
bandwidth = [KernelDensity.default_bandwidth(X[:, t]) for t in 1:T]
grid_lo = [first(k.x) for k in kdes]
grid_step = [step(k.x) for k in kdes]
density = zeros(T, K)
for t in 1:T; density[t, :] .= kdes[t].density; end
pdf_q = [pdf(kdes[t], Xq[i, t]) for i in 1:Nq, t in 1:T]

# the fit (the reference takes the matrix with one ROW per time point) and the encode step
kd, minxs, scales, cvs = init_sahand_legendre_time_dependent(permutedims(X), zeros(Int, N); opts=opts)
cvecs = zeros(T, d, d)
for t in 1:T; cvecs[t, :, :] .= cvs[t]; end
phi_q = zeros(Nq, T, d)
for i in 1:Nq, t in 1:T
    phi_q[i, t, :] .= sahand_legendre_encode(Xq[i, t], d, t, kd, minxs, scales, cvs)
end

# the time-independent form on range(a, b, S)
a, b = -1.0, 1.0
xs_all = X[:]
xs_all = xs_all[@. a <= xs_all <= b]
kall = kde(xs_all)
xs_samps = range(a, b, max(200, T))
f0 = sqrt.(max.(pdf(kall, xs_samps), 0))
ti_minx, ti_scale = remove_zeros!(xs_samps, f0)
ti_cvecs = sahand_legendre_coeffs(xs_samps, f0, d)

out = joinpath(dir, "juliaref_kde.npz")
npzwrite(out, Dict("X" => X, "Xq" => Xq, "d" => [d], "bandwidth" => bandwidth, "grid_lo" => grid_lo, "grid_step" => grid_step,
                   "density" => density, "pdf_q" => pdf_q, "minxs" => Float64.(minxs), "scales" => Float64.(scales), "cvecs" => cvecs,
                   "phi_q" => phi_q, "ti_minx" => [ti_minx], "ti_scale" => [ti_scale], "ti_cvecs" => ti_cvecs))
println("wrote ", out)
