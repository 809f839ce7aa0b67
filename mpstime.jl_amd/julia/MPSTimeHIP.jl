# MPSTimeHIP.jl - Julia shim that plugs libmpstime_hip.so in as the sweep engine of MPSTime.jl.
#
# The seam is the method the reference selects at src/Training/RealRealHighDimension.jl:556-560,
#     fitMPS(W::MPS, training_states_meta, testing_states_meta, opts)        (:587-890)
# next to the existing `use_legacy_ITensor` switch.  Everything above it (options, preprocessing,
# encodings, generate_startingMPS) and below it (TrainedMPS, classify) stays Julia; `impute_batch` at the end is the
# device-side body of the imputation loop (get_predictions, src/Imputation/imputation.jl:264-410).
#
# Julia is not installed in the build container or on the GPU box (SURVEY.md fact 3), so this file
# has been written to the C ABI in include/mpstime_hip.h but never executed; the Python mirror in
# mpstime.jl_amd/ drives the identical ABI and is what the tests run.  Every ITensors name used below exists in
# ITensors 0.6.22 (the reference's pin): MPS, siteinds via MPSTime.get_siteinds, linkinds, dim, array, itensor, Index.
# First run with Julia: `julia --project=<MPSTime.jl> mpstime.jl_amd/julia/roundtrip_check.jl <MPSTime.jl> --shim`
# trains one small model through this shim and prints the content digest the Python mirror prints for the same inputs.
module MPSTimeHIP

using ITensors          # the reference's only tensor dependency (src/MPSTime.jl:9, Project.toml:50 pins ITensors = 0.6.22, which still
                        # carries MPS / siteinds / linkinds itself; ITensorMPS is NOT a dependency of MPSTime.jl)
import MPSTime
import MPSTime: EncodedTimeSeriesSet, PState, AbstractMPSOptions, MPSOptions, Options, TrainedMPS,
                safe_options, find_label, get_siteinds, KLDLoss, MSELoss, BBOpt

const LIB = get(ENV, "MPSTIME_HIP_LIB", "libmpstime_hip.so")
const MPST_ABI_VERSION = 2      # include/mpstime_hip.h this file was written against

function __init__()
    v = ccall((:mpst_version, LIB), Cint, ())
    v == MPST_ABI_VERSION || error("libmpstime_hip.so implements ABI version $v, MPSTimeHIP.jl was written for $MPST_ABI_VERSION")
end

# mpst_set_dataset's dtype: the element type everything crosses the boundary in (opts.dtype, RealRealHighDimension.jl:442)
dtype_code(::Type{Float64}) = Int32(0)
dtype_code(::Type{Float32}) = Int32(1)
dtype_code(::Type{ComplexF64}) = Int32(2)
dtype_code(::Type{ComplexF32}) = Int32(3)

struct MpstOptions            # mpst_options, field for field
    chi_max::Int32; update_iters::Int32; loss::Int32; optimiser::Int32
    rescale_before::Int32; rescale_after::Int32; train_classes_separately::Int32
    svd_alg::Int32; rebuild_caches::Int32; track_cost::Int32
    eta::Float64; cutoff::Float64
end
struct MpstSweepStats
    seconds::Float64; svd_status::Int32; max_chi::Int32; eig_sweeps_total::Int32; eig_fallbacks::Int32
end

const MPST_ERR_UNSUPPORTED = -2
const MPST_ERR_SVD = -4

"""Which librccl the library bound (it is loaded at run time, never linked): `(path_and_how, version, built_against)`."""
function comm_library()
    buf = Vector{UInt8}(undef, 1024)
    ver = Ref{Int32}(0); built = Ref{Int32}(0)
    ccall((:mpst_comm_library, LIB), Cint, (Ptr{UInt8}, Int32, Ref{Int32}, Ref{Int32}), buf, Int32(length(buf)), ver, built)
    return (unsafe_string(pointer(buf)), Int(ver[]), Int(built[]))
end

function check(ctx, rc)
    rc == 0 && return
    msg = unsafe_string(ccall((:mpst_last_error, LIB), Cstring, (Ptr{Cvoid},), ctx))
    rc == MPST_ERR_SVD && throw(ArgumentError(msg))          # the class tune() retries on (tuning.jl:73-86)
    rc == MPST_ERR_UNSUPPORTED && error(msg)                 # loss_functions.jl:166-170
    error("mpstime_hip [$rc]: $msg")
end

"EncodedTimeSeriesSet -> (phi[d,T,N] in the element type E, label_idx 0-based Int32)"
function pack_states(ets::EncodedTimeSeriesSet, d, T, ::Type{E}) where {E}
    N = length(ets.timeseries)
    phi = Array{E}(undef, d, T, N)
    lab = Vector{Int32}(undef, N)
    for (i, ps) in enumerate(ets.timeseries)
        for t in 1:T
            phi[:, t, i] .= ps.pstate[t]
        end
        lab[i] = Int32(ps.label_index) - 1
    end
    return phi, lab
end

"Site tensors in the boundary layout: column-major (s, l_left, l_right[, label])."
function pack_mps(W::MPS, ::Type{E}) where {E}
    T = length(W)
    pos, label_idx = find_label(W)
    sites = get_siteinds(W)
    links = linkinds(W)
    bufs = Vector{Array{E}}(undef, T)
    chi = ones(Int32, T + 1)
    for j in 1:T
        inds_j = Index[sites[j]]
        j > 1 && push!(inds_j, links[j-1]);  j > 1 && (chi[j] = dim(links[j-1]))
        j < T && push!(inds_j, links[j])
        j == pos && push!(inds_j, label_idx)
        A = E.(array(W[j], inds_j...))
        dl, dr = j > 1 ? dim(links[j-1]) : 1, j < T ? dim(links[j]) : 1
        bufs[j] = reshape(A, dim(sites[j]), dl, dr, (j == pos ? dim(label_idx) : 1))
    end
    return bufs, chi, pos - 1, label_idx, sites
end

function fitMPS_hip(W::MPS, train::EncodedTimeSeriesSet, test::EncodedTimeSeriesSet, opts::AbstractMPSOptions; device::Int=0)
    opts = safe_options(opts)
    T = length(W); d = opts.d
    E = opts.dtype                      # Float64 | Float32 | ComplexF64 | ComplexF32
    verbosity = opts.verbosity
    pos, label_idx = find_label(W)
    C = dim(label_idx)
    nsweeps = opts.nsweeps
    # a loss / an optimiser, or one per sweep (RealRealHighDimension.jl:693-713; same messages)
    if opts.loss_grad isa AbstractArray
        @assert length(opts.loss_grad) == nsweeps "loss_grad(...)::(loss,grad) must be a loss function or an array of loss functions with length nsweeps"
        loss_grads = opts.loss_grad
    elseif opts.loss_grad isa Function
        loss_grads = [opts.loss_grad for _ in 1:nsweeps]
    else
        error("loss_grad(...)::(loss,grad) must be a loss function or an array of loss functions with length nsweeps")
    end
    if opts.train_classes_separately && !(eltype(loss_grads) <: KLDLoss)                                       # :702-704
        @warn "Classes will be trained separately, but the cost function _may_ depend on measurements of multiple classes. Switch to a KLD style cost function or ensure your custom cost function depends only on one class at a time."
    end
    if opts.bbopt isa AbstractArray
        @assert length(opts.bbopt) == nsweeps "bbopt must be an optimiser or an array of optimisers to use with length nsweeps"
        bbopts = opts.bbopt
    elseif opts.bbopt isa BBOpt
        bbopts = [opts.bbopt for _ in 1:nsweeps]
    else
        error("bbopt must be an optimiser or an array of optimisers to use with length nsweeps")
    end
    loss_code(lg) = lg isa KLDLoss ? 0 : lg isa MSELoss ? 1 : -1            # -1: the library answers MPST_ERR_UNSUPPORTED
    optim_code(bb) = bb.name == "CustomGD" ? (uppercase(bb.fl) == "TSGO" ? 0 : 1) : -1
    sweep_options(its) = MpstOptions(opts.chi_max, opts.update_iters, loss_code(loss_grads[its]), optim_code(bbopts[its]), opts.rescale[1],
                                     opts.rescale[2], opts.train_classes_separately, opts.svd_alg == "recursive" ? 1 : 0, 0,
                                     opts.track_cost ? 1 : 0, opts.eta, opts.cutoff)
    ctx = Ref{Ptr{Cvoid}}(C_NULL)
    check(C_NULL, ccall((:mpst_create, LIB), Cint, (Ref{Ptr{Cvoid}}, Cint), ctx, device))
    c = ctx[]
    try
        check(c, ccall((:mpst_set_options, LIB), Cint, (Ptr{Cvoid}, Ref{MpstOptions}), c, sweep_options(1)))
        for (which, ets) in ((0, train), (1, test))
            isempty(ets.timeseries) && continue
            phi, lab = pack_states(ets, d, T, E)
            check(c, ccall((:mpst_set_dataset, LIB), Cint,
                  (Ptr{Cvoid}, Cint, Ptr{Cvoid}, Ptr{Int32}, Int64, Int32, Int32, Int32, Int32, Ptr{Int64}),
                  c, which, phi, lab, length(lab), T, d, C, dtype_code(E), C_NULL))
        end
        bufs, chi, ls, _, sites = pack_mps(W, E)
        check(c, ccall((:mpst_set_mps, LIB), Cint, (Ptr{Cvoid}, Ptr{Ptr{Cvoid}}, Ptr{Int32}, Int32, Int32),
              c, [pointer(b) for b in bufs], chi, T, ls))
        verbosity > -1 && println("Using $(opts.update_iters) iterations per update.")                      # :629
        check(c, ccall((:mpst_build_caches, LIB), Cint, (Ptr{Cvoid},), c))

        has_test = !isempty(test.timeseries)
        info = Dict{String,Vector}("train_loss" => Float64[], "train_acc" => Float64[], "test_loss" => Float64[],
                                   "time_taken" => Float64[], "train_KL_div" => Float64[])
        has_test && merge!(info, Dict("test_acc" => Float64[], "test_KL_div" => Float64[], "test_conf" => Matrix{Float64}[]))
        function log!(t)
            opts.log_level > 0 || return NaN
            mse = Ref(0.0); kld = Ref(0.0); acc = Ref(0.0); conf = zeros(Int64, C, C)
            check(c, ccall((:mpst_eval, LIB), Cint, (Ptr{Cvoid}, Cint, Ref{Float64}, Ref{Float64}, Ref{Float64}, Ptr{Int64}), c, 0, mse, kld, acc, conf))
            push!(info["train_loss"], mse[]); push!(info["train_acc"], acc[]); push!(info["time_taken"], t); push!(info["train_KL_div"], kld[])
            verbosity > -1 && println("Training KL Div. $(kld[]) | Training acc. $(acc[]).")                  # :679-684, :835-840
            if has_test
                check(c, ccall((:mpst_eval, LIB), Cint, (Ptr{Cvoid}, Cint, Ref{Float64}, Ref{Float64}, Ref{Float64}, Ptr{Int64}), c, 1, mse, kld, acc, conf))
                push!(info["test_loss"], mse[]); push!(info["test_acc"], acc[]); push!(info["test_KL_div"], kld[])
                push!(info["test_conf"], permutedims(Float64.(conf)))     # C row-major [truth][pred] -> Julia [truth, pred]
                if verbosity > -1
                    println("Test KL Div. $(kld[]) | Testing acc. $(acc[]).")
                    println("")
                    println("Test conf: $(info["test_conf"][end]).")                                          # :685
                end
            end
            return acc[]
        end
        log!(0.0)
        nb = T - 1
        trace = zeros(Float64, opts.update_iters + 1, 2nb)
        for its in 1:nsweeps
            verbosity > -1 && println("Using optimiser $(bbopts[its].name) with the \"$(bbopts[its].fl)\" algorithm")   # :728
            verbosity > -1 && println("Starting backward sweeep: [$its/$nsweeps]")                                      # :729
            # this sweep's loss / optimiser (:727-728 index loss_grads[itS], bbopts[itS])
            its > 1 && check(c, ccall((:mpst_set_options, LIB), Cint, (Ptr{Cvoid}, Ref{MpstOptions}), c, sweep_options(its)))
            st = Ref(MpstSweepStats(0, 0, 0, 0, 0))
            check(c, ccall((:mpst_sweep, LIB), Cint, (Ptr{Cvoid}, Ref{MpstSweepStats}), c, st))
            # both half-sweeps run inside the one call: the reference's mid-sweep lines (:766, :772) go where they fall in its output -
            # between the two halves' per-bond lines when those are printed, straight after the call otherwise
            midlines() = if verbosity > -1
                println("Backward sweep finished.")                                                                    # :766
                println("Starting forward sweep: [$its/$nsweeps]")                                                     # :772
            end
            if opts.track_cost && verbosity >= 1
                # what custGD / TSGO (loss_functions.jl:50-52, :80-82) and apply_update (:181-184) print, bond by bond
                check(c, ccall((:mpst_get_loss_trace, LIB), Cint, (Ptr{Cvoid}, Ptr{Float64}), c, trace))
                for q in 1:2nb
                    q == nb + 1 && midlines()
                    lid = q <= nb ? nb - q + 1 : q - nb
                    for it in 1:opts.update_iters
                        println("Loss before step $it: $(trace[it, q])")
                    end
                    println("Loss at site $lid*$(lid+1): $(trace[end, q])")
                end
            else
                midlines()
            end
            verbosity > -1 && println("Finished sweep $its. Time for sweep: $(round(st[].seconds, digits=2))s")        # :811
            acc = log!(st[].seconds)
            opts.exit_early && acc == 1.0 && break
        end
        check(c, ccall((:mpst_normalize, LIB), Cint, (Ptr{Cvoid},), c))
        verbosity > -1 && println("\nMPS normalised!\n")                                                             # :853
        log!(NaN)

        # read the MPS back into ITensors (label back on site T after the forward half-sweep)
        chi_out = zeros(Int32, T + 1); ls_out = Ref{Int32}(0)
        check(c, ccall((:mpst_get_chi, LIB), Cint, (Ptr{Cvoid}, Ptr{Int32}, Ref{Int32}), c, chi_out, ls_out))
        outs = [Array{E}(undef, d, chi_out[j], chi_out[j+1], (j - 1 == ls_out[] ? C : 1)) for j in 1:T]
        check(c, ccall((:mpst_get_mps, LIB), Cint, (Ptr{Cvoid}, Ptr{Ptr{Cvoid}}), c, [pointer(b) for b in outs]))
        links = [Index(Int(chi_out[j+1]), "Link,l=$j") for j in 1:T-1]
        Wn = MPS(T)
        for j in 1:T
            is = Index[sites[j]]
            j > 1 && push!(is, links[j-1]); j < T && push!(is, links[j]); (j - 1 == ls_out[]) && push!(is, label_idx)
            Wn[j] = itensor(reshape(outs[j], dim.(is)...), is...)
        end
        return TrainedMPS(Wn, MPSOptions(opts), train), info, test
    finally
        ccall((:mpst_destroy, LIB), Cvoid, (Ptr{Cvoid},), c)
    end
end

# ---- imputation (src/Imputation/imputation.jl:264-410: the body of get_predictions' instance loop) ----------------------
struct MpstImputeOpts            # mpst_impute_opts
    method::Int32                # 0 median, 1 mode, 2 ITS (rejection_threshold = :none), 3 mean, 4 ITS with rejection
    order::Int32                 # 0 :forwards, 1 :backwards
    get_err::Int32               # get_wmad / get_std
    max_trials::Int32
    mean_basis::Int32            # 0 :Legendre_Norm, 1 :Legendre_No_Norm, 2 :Fourier
    grid_per_site::Int32         # 0: xvals_enc (d, ngrid) shared by all sites, 1: (d, ngrid, T), one table per site
    rejection_threshold::Float64
end
struct MpstImputeModel           # mpst_impute_model
    N::Int64; T::Int32; d::Int32; C::Int32; label_site::Int32
    dtype::Int32                 # 0 Float64, 1 ComplexF64 (site tensors, phi and the grid states alike)
    compute::Int32               # 0 fp64, 1 fp32 chain contractions (densities stay fp64)
    site::Ptr{Ptr{Cvoid}}; chi::Ptr{Int32}; phi::Ptr{Cvoid}; label_idx::Ptr{Int32}
end
# the mpst_impute_model of packed sites (label_site 0-based; phi / label_idx may be nothing); the caller GC.@preserve's what it points into
impute_model_ref(ptrs, chi, N, T, d, C, label_site, cx, compute, phi, label_idx) =
    Ref(MpstImputeModel(N, T, d, C, label_site, cx ? 1 : 0, compute, pointer(ptrs), pointer(chi),
                        phi === nothing ? C_NULL : Ptr{Cvoid}(pointer(phi)), label_idx === nothing ? Ptr{Int32}(C_NULL) : pointer(label_idx)))

"""
    impute_batch(sites, chi, label_site, phi, label_idx, missing, xvals, xvals_enc; method, order, ...)

Every instance of `phi` ((d, T, N), encoded known values; the columns of `missing` ((T, N), UInt8) mark what is to be imputed)
with the class MPS of its label, on the GPU.  `sites[j]` is `Array(mps[j], s_j, l_{j-1}, l_j[, label])`, `xvals` /
`xvals_enc` ((d, ngrid)) are `imp.x_guess_range`.  Returns `(x, err)`, both (T, N), in the encoding's domain;
`invert_test_transform` (src/utils.jl:299) stays with the caller.

`num_trajectories = K` (impute_ITS's keyword, src/Imputation/MPS_methods.jl:304-347; methods 2 and 4 only): every instance is
conditioned once and K chains are sampled from it; `x` and `err` are then (T, K, N).  The uniform numbers are `u`
((max_trials, T, K, N)) or, with `u === nothing`, come from the device generator under `rseed`, keyed by `row_id` (the caller's
row of every instance, default 0:N-1) so that a subset or a permutation of the rows draws the same chains.

`levels` (up to 16 numbers inside (0, 1)) and / or `cdf_stride = s >= 1` (method 0 only; get_cdfs, src/Imputation/imputation.jl:581-622):
returns `(x, err, q, cdf)` with `q` (nq, T, N) the grid value at every level of every missing site's conditional cdf (0 at known
sites) and `cdf` (ncdf, cdf_rows, N), ncdf = (ngrid - 2) ÷ s + 2, that cdf at the grid indices 0, s, 2s, ... and ngrid - 1 for the
r-th missing site of the instance in ascending order (`nothing` for whichever was not asked for).
"""
function impute_batch(sites::Vector{<:Array}, chi::Vector{Int32}, label_site::Integer, phi::Array, label_idx::Vector{Int32},
                      missing::Matrix{UInt8}, xvals::Vector{Float64}, xvals_enc::Matrix;
                      method::Integer=0, order::Integer=0, get_err::Bool=true, max_trials::Integer=10, rejection_threshold::Float64=0.0,
                      u::Union{Nothing,Array{Float64}}=nothing, compute::Integer=0, device::Integer=0,
                      num_trajectories::Union{Nothing,Integer}=nothing, rseed::Integer=0,
                      row_id::Union{Nothing,Vector{Int64}}=nothing,
                      levels::Union{Nothing,Vector{Float64}}=nothing, cdf_stride::Integer=0)
    d, T, N = size(phi)
    cx = eltype(phi) <: Complex
    ctx = Ref{Ptr{Cvoid}}(C_NULL)
    check(C_NULL, ccall((:mpst_create, LIB), Cint, (Ref{Ptr{Cvoid}}, Cint), ctx, device))
    c = ctx[]
    try
        ptrs = [Ptr{Cvoid}(pointer(a)) for a in sites]
        K = num_trajectories === nothing ? 1 : Int(num_trajectories)
        x = num_trajectories === nothing ? zeros(Float64, T, N) : zeros(Float64, T, K, N)
        err = zeros(Float64, size(x)...); secs = Ref(0.0)
        GC.@preserve sites ptrs chi phi label_idx begin
            model = impute_model_ref(ptrs, chi, N, T, d, maximum(label_idx) + 1, label_site - 1, cx, compute, phi, label_idx)
            o = Ref(MpstImputeOpts(method, order, get_err ? 1 : 0, max_trials, cx ? 2 : 1, 0, rejection_threshold))
            if levels !== nothing || cdf_stride > 0
                nq = levels === nothing ? 0 : length(levels)
                rows = cdf_stride > 0 ? Int(maximum(sum(missing .!= 0, dims=1))) : 0
                q = nq > 0 ? zeros(Float64, nq, T, N) : nothing
                cdf = cdf_stride > 0 ? zeros(Float64, (length(xvals) - 2) ÷ cdf_stride + 2, rows, N) : nothing
                check(c, ccall((:mpst_impute_model_dist, LIB), Cint,
                               (Ptr{Cvoid}, Ref{MpstImputeModel}, Ptr{UInt8}, Ptr{Float64}, Ptr{Cvoid}, Int32, Ref{MpstImputeOpts}, Ptr{Float64},
                                Ptr{Float64}, Ref{Float64}, Int32, Ptr{Float64}, Ptr{Float64}, Int32, Int32, Ptr{Float64}),
                               c, model, missing, xvals, xvals_enc, length(xvals), o, x, err, secs, nq,
                               nq > 0 ? pointer(levels) : C_NULL, nq > 0 ? pointer(q) : C_NULL, cdf_stride, rows,
                               cdf_stride > 0 ? pointer(cdf) : C_NULL))
                return x, err, q, cdf
            end
            if num_trajectories !== nothing
                check(c, ccall((:mpst_impute_model_traj, LIB), Cint,
                               (Ptr{Cvoid}, Ref{MpstImputeModel}, Ptr{UInt8}, Ptr{Float64}, Ptr{Cvoid}, Int32, Ref{MpstImputeOpts}, Int32,
                                Ptr{Float64}, Int64, Ptr{Int64}, Ptr{Float64}, Ptr{Float64}, Ref{Float64}),
                               c, model, missing, xvals, xvals_enc, length(xvals), o, K, u === nothing ? C_NULL : pointer(u),
                               reinterpret(Int64, UInt64(rseed)), row_id === nothing ? C_NULL : pointer(row_id), x, err, secs))
                return x, err
            end
            check(c, ccall((:mpst_impute_model_run, LIB), Cint,
                           (Ptr{Cvoid}, Ref{MpstImputeModel}, Ptr{UInt8}, Ptr{Float64}, Ptr{Cvoid}, Int32, Ref{MpstImputeOpts}, Ptr{Float64},
                            Ptr{Float64}, Ptr{Float64}, Ref{Float64}),
                           c, model, missing, xvals, xvals_enc, length(xvals), o, u === nothing ? C_NULL : pointer(u), x, err, secs))
        end
        return x, err
    finally
        ccall((:mpst_destroy, LIB), Cvoid, (Ptr{Cvoid},), c)
    end
end

"""
    impute_dist(c, which, missing, xvals, xvals_enc; order, get_err, levels, cdf_stride)

The same outputs on a context `c` that holds the trained MPS and data set `which` (0 train, 1 test), as `mpst_impute` takes them
(real models; `xvals_enc` is (d, ngrid) Float64).  Returns `(x, err, q, cdf)` as `impute_batch` does.
"""
function impute_dist(c::Ptr{Cvoid}, which::Integer, missing::Matrix{UInt8}, xvals::Vector{Float64}, xvals_enc::Matrix{Float64};
                     order::Integer=0, get_err::Bool=true, levels::Union{Nothing,Vector{Float64}}=nothing, cdf_stride::Integer=0)
    T, N = size(missing)
    nq = levels === nothing ? 0 : length(levels)
    rows = cdf_stride > 0 ? Int(maximum(sum(missing .!= 0, dims=1))) : 0
    x = zeros(Float64, T, N); err = zeros(Float64, T, N); secs = Ref(0.0)
    q = nq > 0 ? zeros(Float64, nq, T, N) : nothing
    cdf = cdf_stride > 0 ? zeros(Float64, (length(xvals) - 2) ÷ cdf_stride + 2, rows, N) : nothing
    o = Ref(MpstImputeOpts(0, order, get_err ? 1 : 0, 1, 1, 0, 0.0))
    check(c, ccall((:mpst_impute_dist, LIB), Cint,
                   (Ptr{Cvoid}, Cint, Ptr{UInt8}, Ptr{Float64}, Ptr{Float64}, Int32, Ref{MpstImputeOpts}, Ptr{Float64}, Ptr{Float64},
                    Ref{Float64}, Int32, Ptr{Float64}, Ptr{Float64}, Int32, Int32, Ptr{Float64}),
                   c, which, missing, xvals, xvals_enc, length(xvals), o, x, err, secs, nq,
                   nq > 0 ? pointer(levels) : C_NULL, nq > 0 ? pointer(q) : C_NULL, cdf_stride, rows,
                   cdf_stride > 0 ? pointer(cdf) : C_NULL))
    return x, err, q, cdf
end

# ---- Sahand-Legendre encodings on the device ----------------------------------------------------------------------------------
struct MpstEncodeOpts            # mpst_encode_opts
    basis::Int32
    sigmoid_transform::Int32
    minmax::Int32
    is_test::Int32
    rescale_out_of_bounds::Int32
    fit_sigmoid::Int32
    median::Float64
    iqr::Float64
    lo::Float64
    hi::Float64
    data_lb::Float64
    data_ub::Float64
    range_a::Float64
    range_b::Float64
end
struct MpstKdeOpts               # mpst_kde_opts
    npoints::Int32               # K grid points of every density estimate
    per_site::Int32              # 0: one table for all sites, 1: T tables
    lo::Ptr{Float64}             # (S,), S = per_site == 1 ? T : 1
    step::Ptr{Float64}           # (S,)
    coef::Ptr{Float64}           # (K + 2, S): the quadratic B-spline coefficients of site s in column s
    minx::Ptr{Float64}           # (S,)
    scale::Ptr{Float64}          # (S,)
    cvecs::Ptr{Float64}          # (d, d, S): cvecs[i, n, s] multiplies x^(i-1) in function n of site s (the reference's cVecs[s][n, i])
end

"""
    encode_kde_values(X, d, lo, step, coef, minx, scale, cvecs; per_site, device)

The Sahand-Legendre states of the values `X` ((T, N), already in the encoding's range) from the fitted tables
(`mpst_encode_kde_values`, no preprocessing): `lo`, `step`, `minx`, `scale` (S,), `coef` (K + 2, S) and `cvecs` (d, d, S) with
S = T (`per_site`) or 1 - column-major arrays, so site s is contiguous as the C side reads it.  Returns `phi` (d, T, N).
"""
function encode_kde_values(X::Matrix{Float64}, d::Integer, lo::Vector{Float64}, step::Vector{Float64}, coef::Matrix{Float64},
                           minx::Vector{Float64}, scale::Vector{Float64}, cvecs::Array{Float64,3}; per_site::Bool=true, device::Integer=0)
    T, N = size(X)
    S = per_site ? T : 1
    K = size(coef, 1) - 2
    (length(lo), length(step), length(minx), length(scale), size(coef, 2), size(cvecs)) == (S, S, S, S, S, (d, d, S)) ||
        throw(ArgumentError("the tables must hold one entry per site (or one in all): S = $S"))
    phi = zeros(Float64, d, T, N)
    secs = Ref(0.0)
    with_context(device) do c
        eo = Ref(MpstEncodeOpts(1, 0, 0, 0, 0, 0, 0.0, 0.0, 0.0, 1.0, 0.0, 1.0, 0.0, 1.0))      # no transforms, identity range map
        kd = Ref(MpstKdeOpts(K, per_site ? 1 : 0, pointer(lo), pointer(step), pointer(coef), pointer(minx), pointer(scale), pointer(cvecs)))
        GC.@preserve X lo step coef minx scale cvecs eo kd begin
            check(c, ccall((:mpst_encode_kde_values, LIB), Cint,
                           (Ptr{Cvoid}, Ptr{Float64}, Int64, Int32, Int32, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float64}, Ref{Float64}),
                           c, X, N, T, d, Base.unsafe_convert(Ptr{Cvoid}, eo), Base.unsafe_convert(Ptr{Cvoid}, kd), phi, C_NULL, secs))
        end
    end
    return phi
end

# ---- projected bases on the device --------------------------------------------------------------------------------------------
struct MpstProjOpts              # mpst_proj_opts
    basis::Int32                 # 0 legendre(norm = true), 1 legendre_no_norm, 2 fourier
    orders::Ptr{Int32}           # (d, T): column t holds site t's Legendre orders or signed Fourier frequencies
    inv_norm::Ptr{Float64}       # (T,): 1 / sqrt(Pl(1, m; normalized) m), m the site's largest order; read for basis 0 only, else C_NULL
    max_order::Int32             # bounds every |orders[j, t]|
end

# the checks the library cannot make (it sees pointers, not lengths) and the struct; preserve `orders` and `inv_norm` over the call
function proj_opts(basis::Integer, orders::Matrix{Int32}, inv_norm::Union{Nothing,Vector{Float64}}, d::Integer, T::Integer)
    size(orders) == (d, T) || throw(ArgumentError("orders must be (d, T) = ($d, $T), got $(size(orders))"))
    isnothing(inv_norm) || length(inv_norm) == T || throw(ArgumentError("inv_norm must hold one entry per site"))
    return MpstProjOpts(basis, pointer(orders), isnothing(inv_norm) ? Ptr{Float64}(C_NULL) : pointer(inv_norm), maximum(abs, orders))
end

"""
    encode_proj_values(X, orders; basis, inv_norm, device)

The projected-basis states of the values `X` ((T, N), already in (-1, 1)) from the order lists the fit selected
(`mpst_encode_proj_values`, no preprocessing).  `orders` is (d, T): for `basis` 0 / 1 (projected `legendre(norm=true)` /
`legendre_no_norm`) the Legendre orders that are evaluated - the reference's `legendre_encode(x, nds, ds)` evaluates `Pl(x, p)`
for the selected position `p`, so `orders = ds` -, for `basis` 2 (projected `fourier`) the signed frequencies
`get_fourier_freqs(10d)[ds]`.  Returns `phi` (d, T, N), `Float64` or, for `basis` 2, `ComplexF64`.
"""
function encode_proj_values(X::Matrix{Float64}, orders::Matrix{Int32}; basis::Integer=1, inv_norm::Union{Nothing,Vector{Float64}}=nothing,
                            device::Integer=0)
    T, N = size(X)
    d = size(orders, 1)
    phi = zeros(basis == 2 ? ComplexF64 : Float64, d, T, N)
    secs = Ref(0.0)
    with_context(device) do c
        eo = Ref(MpstEncodeOpts(1, 0, 0, 0, 0, 0, 0.0, 0.0, 0.0, 1.0, 0.0, 1.0, 0.0, 1.0))      # no transforms, identity range map
        GC.@preserve X orders inv_norm eo begin
            pj = Ref(proj_opts(basis, orders, inv_norm, d, T))
            check(c, ccall((:mpst_encode_proj_values, LIB), Cint,
                           (Ptr{Cvoid}, Ptr{Float64}, Int64, Int32, Int32, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float64}, Ref{Float64}),
                           c, X, N, T, d, Base.unsafe_convert(Ptr{Cvoid}, eo), Base.unsafe_convert(Ptr{Cvoid}, pj), phi, C_NULL, secs))
        end
    end
    return phi
end

"""
    encode_proj_dataset!(c, which, X, labels, C, eo, orders; basis, inv_norm)

`mpst_encode_proj_dataset` on the context `c`: the raw series `X` ((T, N), sorted by class, `labels` 0-based) go through the
preprocessing `eo` describes and the projected basis, and become data set `which` (0 train, 1 test) of the context.  `eo` comes back
with what a training set fitted (median, iqr, lo, hi): hand it on, with `is_test = 1`, for the test set.  Returns the device seconds.
"""
function encode_proj_dataset!(c::Ptr{Cvoid}, which::Integer, X::Matrix{Float64}, labels::Vector{Int32}, C::Integer, eo::Ref{MpstEncodeOpts},
                              orders::Matrix{Int32}; basis::Integer=1, inv_norm::Union{Nothing,Vector{Float64}}=nothing)
    T, N = size(X)
    d = size(orders, 1)
    length(labels) == N || throw(ArgumentError("one label per series"))
    secs = Ref(0.0)
    GC.@preserve X labels orders inv_norm eo begin
        pj = Ref(proj_opts(basis, orders, inv_norm, d, T))
        check(c, ccall((:mpst_encode_proj_dataset, LIB), Cint,
                       (Ptr{Cvoid}, Cint, Ptr{Float64}, Ptr{Int32}, Int64, Int32, Int32, Int32, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Int64}, Ptr{Float64},
                        Ref{Float64}),
                       c, which, X, labels, N, T, d, C, Base.unsafe_convert(Ptr{Cvoid}, eo), Base.unsafe_convert(Ptr{Cvoid}, pj), C_NULL, C_NULL, secs))
    end
    return secs[]
end

# ---- leave-one-out site conditionals ----------------------------------------------------------------------------------------
struct MpstSiteCondOpts          # mpst_sitecond_opts
    grid_per_site::Int32         # 0: xvals_enc (d, ngrid) shared by all sites, 1: (d, ngrid, T), one table per site
    get_err::Int32
    nq::Int32
    reserved::Int32
    levels::Ptr{Float64}
end

"""
    site_conditionals(sites, chi, label_site, phi, label_idx, x, xvals, xvals_enc; get_err, levels, device)

For every COMPLETE series of `phi` ((d, T, N), its values `x` (T, N) in the encoding's domain) and every site t the distribution of
x_t given all the other values, under the class MPS of its label (`mpst_site_conditionals`; arguments as `impute_batch` takes them,
`xvals_enc` (d, ngrid) or (d, ngrid, T)).  Returns `(nll, pit, median, err, q)`: (T, N) arrays - the negative log conditional
density at the observed value, the PIT, the median imputer's value and its WMAD - and `q` (nq, T, N) the grid value at every level
(`nothing` without `levels`).
"""
function site_conditionals(sites::Vector{<:Array}, chi::Vector{Int32}, label_site::Integer, phi::Array, label_idx::Vector{Int32},
                           x::Matrix{Float64}, xvals::Vector{Float64}, xvals_enc::Array;
                           get_err::Bool=true, levels::Union{Nothing,Vector{Float64}}=nothing, device::Integer=0)
    d, T, N = size(phi)
    cx = eltype(phi) <: Complex
    nq = levels === nothing ? 0 : length(levels)
    nll = zeros(Float64, T, N); pit = zeros(Float64, T, N); med = zeros(Float64, T, N); err = zeros(Float64, T, N)
    q = nq > 0 ? zeros(Float64, nq, T, N) : nothing
    secs = Ref(0.0)
    with_context(device) do c
        ptrs = [Ptr{Cvoid}(pointer(a)) for a in sites]
        o = Ref(MpstSiteCondOpts(ndims(xvals_enc) == 3 ? 1 : 0, get_err ? 1 : 0, nq, 0, nq > 0 ? pointer(levels) : Ptr{Float64}(C_NULL)))
        GC.@preserve sites ptrs chi phi label_idx levels o begin
            model = impute_model_ref(ptrs, chi, N, T, d, maximum(label_idx) + 1, label_site - 1, cx, 0, phi, label_idx)
            check(c, ccall((:mpst_site_conditionals, LIB), Cint,
                           (Ptr{Cvoid}, Ref{MpstImputeModel}, Ptr{Float64}, Ptr{Float64}, Ptr{Cvoid}, Int32, Ptr{Cvoid}, Ptr{Float64},
                            Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ref{Float64}),
                           c, model, x, xvals, xvals_enc, length(xvals), Base.unsafe_convert(Ptr{Cvoid}, o), nll, pit, med, err,
                           nq > 0 ? pointer(q) : C_NULL, secs))
        end
    end
    return nll, pit, med, err, q
end

"""
    window_conditionals(sites, chi, label_site, phi, label_idx, max_width; device)

For every COMPLETE series of `phi` ((d, T, N)), every start t and every width w = 1 .. `max_width` that fits, -ln of the Born
probability of the values of the window t .. t+w-1 given all the others, under the class MPS of the series' label
(`mpst_window_conditionals`; model arguments as `site_conditionals` takes them).  Returns `nll` (max_width, T, N): entry
[w, t, i]; NaN where the window would pass the end of the chain.
"""
function window_conditionals(sites::Vector{<:Array}, chi::Vector{Int32}, label_site::Integer, phi::Array, label_idx::Vector{Int32},
                             max_width::Integer; device::Integer=0)
    d, T, N = size(phi)
    cx = eltype(phi) <: Complex
    nll = zeros(Float64, max(max_width, 1), T, N)
    secs = Ref(0.0)
    with_context(device) do c
        ptrs = [Ptr{Cvoid}(pointer(a)) for a in sites]
        GC.@preserve sites ptrs chi phi label_idx begin
            model = impute_model_ref(ptrs, chi, N, T, d, maximum(label_idx) + 1, label_site - 1, cx, 0, phi, label_idx)
            check(c, ccall((:mpst_window_conditionals, LIB), Cint,
                           (Ptr{Cvoid}, Ref{MpstImputeModel}, Int32, Ptr{Float64}, Ref{Float64}),
                           c, model, max_width, nll, secs))
        end
    end
    return nll
end

"""
    marginal_conditionals(sites, chi, label_site, phi, label_idx, missing, x, xvals, xvals_enc; get_err, levels, device)

For every series of `phi` ((d, T, N)) with the sites `missing` ((T, N) UInt8, non-zero: missing) and every site t, known or missing,
the distribution of x_t given the known values of the other sites, the missing ones summed out (Born rule), under the class MPS of
the series' label (`mpst_marginal_conditionals`; model and grid arguments as `site_conditionals` takes them).  `x` (T, N): the value
in the encoding's domain - the held-out true value or NaN at a missing site, where `phi` is read only when it is finite.  Returns
`(nll, pit, median, err, mean, q)`: (T, N) arrays, `nll` and `pit` NaN at missing sites without a value, and `q` (nq, T, N)
(`nothing` without `levels`).
"""
function marginal_conditionals(sites::Vector{<:Array}, chi::Vector{Int32}, label_site::Integer, phi::Array, label_idx::Vector{Int32},
                               missing::Matrix{UInt8}, x::Matrix{Float64}, xvals::Vector{Float64}, xvals_enc::Array;
                               get_err::Bool=true, levels::Union{Nothing,Vector{Float64}}=nothing, device::Integer=0)
    d, T, N = size(phi)
    cx = eltype(phi) <: Complex
    nq = levels === nothing ? 0 : length(levels)
    nll = zeros(Float64, T, N); pit = zeros(Float64, T, N); med = zeros(Float64, T, N); err = zeros(Float64, T, N)
    mean = zeros(Float64, T, N)
    q = nq > 0 ? zeros(Float64, nq, T, N) : nothing
    secs = Ref(0.0)
    with_context(device) do c
        ptrs = [Ptr{Cvoid}(pointer(a)) for a in sites]
        o = Ref(MpstSiteCondOpts(ndims(xvals_enc) == 3 ? 1 : 0, get_err ? 1 : 0, nq, 0, nq > 0 ? pointer(levels) : Ptr{Float64}(C_NULL)))
        GC.@preserve sites ptrs chi phi label_idx levels o begin
            model = impute_model_ref(ptrs, chi, N, T, d, maximum(label_idx) + 1, label_site - 1, cx, 0, phi, label_idx)
            check(c, ccall((:mpst_marginal_conditionals, LIB), Cint,
                           (Ptr{Cvoid}, Ref{MpstImputeModel}, Ptr{UInt8}, Ptr{Float64}, Ptr{Float64}, Ptr{Cvoid}, Int32, Ptr{Cvoid},
                            Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ref{Float64}),
                           c, model, missing, x, xvals, xvals_enc, length(xvals), Base.unsafe_convert(Ptr{Cvoid}, o), nll, pit, med, err,
                           mean, nq > 0 ? pointer(q) : C_NULL, secs))
        end
    end
    return nll, pit, med, err, mean, q
end

# ---- entanglement analysis (src/Analysis/analyse.jl) ---------------------------------------------------------------------
const MPST_ERR_DOMAIN = -6

function check_analysis(ctx, rc)
    rc == MPST_ERR_DOMAIN && throw(DomainError(unsafe_string(ccall((:mpst_last_error, LIB), Cstring, (Ptr{Cvoid},), ctx))))
    check(ctx, rc)
end

function with_context(f, device)
    ctx = Ref{Ptr{Cvoid}}(C_NULL)
    check(C_NULL, ccall((:mpst_create, LIB), Cint, (Ref{Ptr{Cvoid}}, Cint), ctx, device))
    try
        return f(ctx[])
    finally
        ccall((:mpst_destroy, LIB), Cvoid, (Ptr{Cvoid},), ctx[])
    end
end

"(bee, see), each a (T, C) matrix in natural log: mpst_entanglement on the trained model (Float64 only)."
function entanglement(tm::TrainedMPS; device::Integer=0)
    sites, chi, label_site, label_idx, _ = pack_mps(tm.mps, Float64)
    T, d, C = length(sites), size(sites[1], 1), dim(label_idx)
    bee = zeros(Float64, T, C); see = zeros(Float64, T, C)
    with_context(device) do c
        ptrs = [Ptr{Cvoid}(pointer(a)) for a in sites]
        GC.@preserve sites ptrs chi begin
            model = impute_model_ref(ptrs, chi, 0, T, d, C, label_site, false, 0, nothing, nothing)
            check_analysis(c, ccall((:mpst_entanglement, LIB), Cint, (Ptr{Cvoid}, Ref{MpstImputeModel}, Ptr{Float64}, Ptr{Float64}),
                                    c, model, bee, see))
        end
    end
    return bee, see
end

"bipartite_spectrum(mps::TrainedMPS; logfn) (analyse.jl:47-64) on the GPU."
function bipartite_spectrum(tm::TrainedMPS; logfn::Function=log, device::Integer=0)
    logfn in (log, log2, log10) || throw(ArgumentError("logfn must be one of: log, log2, or log10"))
    bee, _ = entanglement(tm; device=device)
    scale = logfn === log ? 1.0 : (logfn === log2 ? 1 / log(2) : 1 / log(10))
    return [bee[:, c] .* scale for c in 1:size(bee, 2)]
end

"single_site_spectrum(mps::TrainedMPS) (analyse.jl:122-138) on the GPU."
function single_site_spectrum(tm::TrainedMPS; device::Integer=0)
    _, see = entanglement(tm; device=device)
    return [see[:, c] for c in 1:size(see, 2)]
end

"""see_variation(mps::TrainedMPS, measure_series, class) (analyse.jl:168-194) on the GPU: the same pre-processing and encoding
(init_imputation_problem, transform_train_data / transform_test_data, get_state), the result indexed [instance, k+1, site]."""
function see_variation(tm::TrainedMPS, measure_series::Matrix, class::Int=0; device::Integer=0)
    imp = MPSTime.init_imputation_problem(tm, measure_series, verbosity=0)
    _, norms = MPSTime.transform_train_data(imp.X_train; opts=imp.opts)
    scaled, _ = MPSTime.transform_test_data(measure_series, norms; opts=imp.opts)
    sites, chi, label_site, label_idx, _ = pack_mps(tm.mps, Float64)
    T, d, C = length(sites), size(sites[1], 1), dim(label_idx)
    N = size(scaled, 1)
    phi = Array{Float64}(undef, d, T, N)
    for i in 1:N, j in 1:T
        phi[:, j, i] .= MPSTime.get_state(scaled[i, j], imp.opts, j, imp.enc_args)
    end
    out = Array{Float64}(undef, T, T, N)            # [site, k, instance] column-major = [instance][k][site] row-major
    secs = Ref(0.0)
    with_context(device) do c
        ptrs = [Ptr{Cvoid}(pointer(a)) for a in sites]
        GC.@preserve sites ptrs chi phi begin
            model = impute_model_ref(ptrs, chi, N, T, d, C, label_site, false, 0, phi, nothing)
            check_analysis(c, ccall((:mpst_see_variation, LIB), Cint, (Ptr{Cvoid}, Ref{MpstImputeModel}, Int32, Ptr{Float64}, Ref{Float64}),
                                    c, model, Int32(class), out, secs))
        end
    end
    return permutedims(out, (3, 2, 1))
end

"""pair_analysis(tm; observable): mutual information, mean and covariance of every pair of sites of each class MPS
(mpst_pair_analysis).  `observable`: a symmetric (d, d) matrix for all sites, a (d, d, T) array with one per site, or `nothing`
(no moments).  Returns (mi, mean, cov): (T, T, C), (T, C) and (T, T, C) arrays, natural log; the diagonal of `mi` holds the
single-site entropies.  `mi` is `nothing` for d > 11."""
function pair_analysis(tm::TrainedMPS; observable::Union{Nothing,Array{Float64}}=nothing, device::Integer=0)
    sites, chi, label_site, label_idx, _ = pack_mps(tm.mps, Float64)
    T, d, C = length(sites), size(sites[1], 1), dim(label_idx)
    per_site = observable !== nothing && ndims(observable) == 3
    obs = observable === nothing ? Float64[] : Array{Float64}(observable)       # symmetric tables: column-major = row-major
    mi = d <= 11 ? zeros(Float64, T, T, C) : Float64[]
    mean = zeros(Float64, T, C); cov = zeros(Float64, T, T, C)
    secs = Ref(0.0)
    with_context(device) do c
        ptrs = [Ptr{Cvoid}(pointer(a)) for a in sites]
        GC.@preserve sites ptrs chi obs mi mean cov begin
            model = impute_model_ref(ptrs, chi, 0, T, d, C, label_site, false, 0, nothing, nothing)
            none = Ptr{Float64}(C_NULL)
            check_analysis(c, ccall((:mpst_pair_analysis, LIB), Cint,
                                    (Ptr{Cvoid}, Ref{MpstImputeModel}, Ptr{Float64}, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ref{Float64}),
                                    c, model, observable === nothing ? none : pointer(obs), Int32(per_site), d <= 11 ? pointer(mi) : none,
                                    observable === nothing ? none : pointer(mean), observable === nothing ? none : pointer(cov), secs))
        end
    end
    return (d <= 11 ? mi : nothing), (observable === nothing ? nothing : mean), (observable === nothing ? nothing : cov)
end

"""model_overlaps(tms; complex=false): the inner products of the class states of the trained models `tms` (mpst_model_overlaps), which
agree in length, physical dimension and label site.  Returns (G, lg, pairs): for the k-th pair (a, b) of `pairs` - every a <= b in row
order, 1-based - `G[c', c, k] * exp(lg[k])` is <psi_{a,c} | psi_{b,c'}> of the label slices as stored (conjugate on a; Cmax x Cmax, zero
beyond the classes of a and b); `lg[k] == -Inf` where the overlap is exactly zero.  The class overlap matrix of get_training_summary is
`abs.(G[:, :, 1])` of one model, divided by the norms sqrt.(diag) on both sides."""
function model_overlaps(tms::Vector{TrainedMPS}; complex::Bool=false, device::Integer=0)
    E = complex ? ComplexF64 : Float64
    K = length(tms)
    packed = [pack_mps(tm.mps, E) for tm in tms]
    sites = [p[1] for p in packed]; chis = [p[2] for p in packed]
    T, d, label_site = length(sites[1]), size(sites[1][1], 1), packed[1][3]
    Cs = [dim(p[4]) for p in packed]
    Cmax = maximum(Cs)
    pairs = [(a, b) for a in 1:K for b in a:K]
    P = length(pairs)
    G = zeros(E, Cmax, Cmax, P)                     # [c', c, pair] column-major = [pair][c][c'] row-major
    lg = zeros(Float64, P)
    secs = Ref(0.0)
    with_context(device) do c
        ptrs = [[Ptr{Cvoid}(pointer(a)) for a in s] for s in sites]
        GC.@preserve sites ptrs chis G lg begin
            models = [MpstImputeModel(0, T, d, Cs[k], label_site, complex ? 1 : 0, 0, pointer(ptrs[k]), pointer(chis[k]), C_NULL, Ptr{Int32}(C_NULL))
                      for k in 1:K]
            GC.@preserve models begin
                check(c, ccall((:mpst_model_overlaps, LIB), Cint,
                               (Ptr{Cvoid}, Ptr{MpstImputeModel}, Int32, Ptr{Int32}, Int32, Ptr{Float64}, Ptr{Float64}, Ref{Float64}),
                               c, pointer(models), Int32(K), Ptr{Int32}(C_NULL), Int32(0), Ptr{Float64}(pointer(G)), pointer(lg), secs))
            end
        end
    end
    return G, lg, pairs
end

end # module
