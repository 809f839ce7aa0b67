# make_analysis_goldens.jl - the reference's own entanglement analysis (src/Analysis/analyse.jl) of its trained ECG200 model, for
# tests/test_analysis_ref.py::test_restatement_against_reference_outputs.  The build image has no Julia, so this script has never
# been executed: it is written against the reference's source for a maintainer who has MPSTime.jl checked out.  Needs MPSTime, JLD2,
# NPZ.
#
#   julia --project=<MPSTime.jl checkout> tests/golden/make_analysis_goldens.jl <repo>/tests/golden
#
# Reads tests/golden/ref_test_dataset.jld2 (the reference's test/Data/ecg200/mps_saves/test_dataset.jld2: the model pinned in
# ref_ecg200_trained_mps.npz) and writes tests/golden/ref_ecg200_analysis.npz:
#   bee_<c>   bipartite_spectrum(mps)[c+1]          (natural log), c = 0, 1
#   see_<c>   single_site_spectrum(mps)[c+1]
#   var_<c>   see_variation(mps, X_train[rows, :], c)  (16, T, T) = [instance, k+1, site], rows = 1:6:91 (0-based 0, 6, ..., 90)
using MPSTime, JLD2, NPZ

dir = ARGS[1]
f = jldopen(joinpath(dir, "ref_test_dataset.jld2"), "r")
mps, X_train = f["mps"], f["X_train"]
close(f)
rows = 1:6:91
out = Dict{String,Any}("rows" => collect(rows) .- 1)
for (c, (b, s)) in enumerate(zip(bipartite_spectrum(mps), single_site_spectrum(mps)))
    out["bee_$(c-1)"] = b
    out["see_$(c-1)"] = s
    out["var_$(c-1)"] = see_variation(mps, X_train[rows, :], c - 1)
end
npzwrite(joinpath(dir, "ref_ecg200_analysis.npz"), out)
println("wrote ", joinpath(dir, "ref_ecg200_analysis.npz"))
