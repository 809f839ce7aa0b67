# make_proj_goldens.jl - pins the projected Legendre bases of this repository (DESIGN.md, "Projected bases") against the Julia
# reference.  The build image has no Julia, so this script has never been executed: it is written against the reference's source
# (file:line below) for a maintainer who has MPSTime.jl checked out.  Needs MPSTime, KernelDensity, LegendrePolynomials, NPZ.
#
#   julia --project=<MPSTime.jl checkout> tests/golden/make_proj_goldens.jl <repo>/tests/golden
#
# Legendre only: projected Fourier cannot run in the reference (no project_fourier(Xs, ys; opts) method, and
# fourier_encode(x, nds, ds::AbstractVector{Integer}) matches no Vector{Int}), so there is nothing of it to record.
# It builds the deterministic training matrix of make_kde_goldens.jl (a closed formula, stored with the results), then writes
# tests/golden/juliaref_proj.npz with
#   X (N, T), Xq (Nq, T), d            the training matrix, the query matrix, the basis dimension
#   wf (T, S)                          construct_kerneldensity_wavefunction (src/Encodings/bases.jl:141-154) of every column over
#                                      range(-1, 1, S), S = max(200, 2N).  The reference takes sqrt.(pdf) unclamped: a DomainError
#                                      here means a slightly negative spline value, which this repository clamps to 0
#   abs2 (T, 7d)                       |c_p|^2 of series_expand (:346-355), recomputed here with the trapezoid rule term by term
#   ds (T, d)                          project_legendre (:385-397): the selected 1-based positions, largest |c_p|^2 first
#   phi_q, phi_q_norm (Nq, T, d)       legendre_encode(x, d, t, ds; norm) (:94-107) of every query value, norm = false / true
# No test reads the file yet: the one that compares mpstime_jl_amd.encodings with it is added in the commit that adds the file.
using MPSTime, KernelDensity, LegendrePolynomials, NPZ
import MPSTime: project_legendre, construct_kerneldensity_wavefunction, legendre_encode, safe_options

dir = ARGS[1]
N, T, Nq, d = 60, 4, 25, 4
X = [clamp(0.55 * sin(1.7 * i + 0.9 * t) + 0.35 * cos(0.37 * i * t) + 0.1, -1.0, 1.0) for i in 1:N, t in 1:T]
Xq = [clamp(0.9 * sin(0.61 * i + 1.3 * t), -1.0, 1.0) for i in 1:Nq, t in 1:T]
opts = safe_options(MPSOptions(; d=d, encoding=:Legendre, verbosity=-1, log_level=0))

# the fit (the reference takes the matrix with one ROW per time point)
ds = project_legendre(permutedims(X), zeros(Int, N); opts=opts)[1]

# its ingredients, site by site
S = max(200, 2N)
wf = zeros(T, S)
c2 = zeros(T, 7d)
for t in 1:T
    xs = X[:, t]
    xs_samps, w = construct_kerneldensity_wavefunction(xs[@. -1.0 <= xs <= 1.0], (-1, 1); max_samples=S)
    wf[t, :] .= w
    for p in 1:7d
        ys = w .* [Pl(x, p - 1; norm=Val(:normalized)) for x in xs_samps]
        c = sum((ys[2:end] .+ ys[1:end-1]) .* 0.5 .* diff(collect(xs_samps)))
        c2[t, p] = abs2(c)
    end
end

phi_q, phi_q_norm = zeros(Nq, T, d), zeros(Nq, T, d)
for i in 1:Nq, t in 1:T
    phi_q[i, t, :] .= legendre_encode(Xq[i, t], d, t, ds; norm=false)
    phi_q_norm[i, t, :] .= legendre_encode(Xq[i, t], d, t, ds; norm=true)
end

dsm = zeros(Int64, T, d)
for t in 1:T; dsm[t, :] .= ds[t]; end
out = joinpath(dir, "juliaref_proj.npz")
npzwrite(out, Dict("X" => X, "Xq" => Xq, "d" => [d], "wf" => wf, "abs2" => c2, "ds" => dsm, "phi_q" => phi_q, "phi_q_norm" => phi_q_norm))
println("wrote ", out)
