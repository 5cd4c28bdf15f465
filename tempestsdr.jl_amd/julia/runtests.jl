# runtests.jl -- replay tests/golden/v2 through the TempestHIP shim (needs Julia, libtempest_hip.so and an MI355X).
#
#     julia tempestsdr.jl_amd/julia/runtests.jl
#
# Expected values: tests/golden/v2/julia (outputs of the reference itself, written by tests/golden/make_golden.jl)
# when present, else tests/golden/v2/oracle (the CPU restatement).  Bit-exact on the frame path, the tolerances
# of tests/test_julia_golden.py on the FFT paths.
#
# STATUS: written without a Julia runtime (none exists in the build container) -- never executed.
using Test

include(joinpath(@__DIR__, "TempestHIP.jl"))
using .TempestHIP

const V2 = normpath(joinpath(@__DIR__, "..", "..", "tests", "golden", "v2"))
const DT = Dict("f32" => Float32, "f64" => Float64, "c64" => ComplexF32, "i32" => Int32, "i64" => Int64, "u64" => UInt64)

function load_all(dir)
    d = Dict{String,Any}()
    for fn in readdir(dir)
        endswith(fn, ".bin") || continue
        parts = split(fn, ".")
        shape = Tuple(parse.(Int, split(parts[3], "x")))
        a = Array{DT[String(parts[2])]}(undef, shape...)
        open(io -> read!(io, a), joinpath(dir, fn))
        d[String(parts[1])] = a
    end
    return d
end

bits(a) = reinterpret(UInt32, vec(collect(Float32, a)))
samebits(a, b) = size(a) == size(b) && bits(a) == bits(b)
relmax(a, b) = maximum(abs.(Float64.(a) .- Float64.(b))) / maximum(abs.(Float64.(b)))

inp = load_all(joinpath(V2, "inputs"))
refdir = isdir(joinpath(V2, "julia")) && !isempty(readdir(joinpath(V2, "julia"))) ? joinpath(V2, "julia") : joinpath(V2, "oracle")
ref = load_all(refdir)
@info "expected values from $refdir"

@testset "TempestHIP vs $(basename(refdir))" begin
    z = inp["iq"]
    @test samebits(amDemod(z), ref["am"])
    @test samebits(invert_amDemod(z), ref["inv_am"])
    @test maximum(abs.(fmDemod(z) .- ref["fm"])) <= 1f-6
    x = inp["rs_in"]
    @test samebits(sig_to_image(x, 30, 40), ref["s2i"])
    @test samebits(sig_to_image(view(x, 1:333), 30, 40), ref["s2i"])          # contiguous view, no copy (GUI.jl:166)
    big = downgradeImage(inp["img_in"])
    @test size(big) == (600, 800)
    @test samebits(vec(big)[1:997:end], ref["down_sub"])
    nv = zeros(Float32, 375); naiveResampler(nv, inp["up_in"], 3)
    @test samebits(nv, ref["naive"])
    resampler! = init_resampler(Float32, 125, 4)
    up = zeros(Float32, 500); resampler!(up, inp["up_in"])
    @test relmax(up, ref["up_out"]) < 1e-5
    @test_throws AssertionError resampler!(up, zeros(Float32, 124))             # Resampler.jl:47
    # vsync: three calls on one SyncXY (stale s_y), indices identical
    sync = SyncXY(zeros(Float32, 77, 131))
    idx = [vsync(inp["vs_img$(k)"], sync) for k in 0:2]
    @test [i[1] for i in idx] == Int.(ref["vs_idx"][:, 1])
    @test [i[2] for i in idx] == Int.(ref["vs_idx"][:, 2])
    @test idx[1][1] == 1
    # autocorrelation / zoom
    Γ, lags = calculate_autocorrelation(inp["ac_x"], 30000.0, 0.0, 0.05)
    @test maximum(abs.(Γ .- ref["ac_db"])) < 2e-4
    @test length(lags) == length(Γ)
    rates, Γz = zoom_autocorr(Γ, 30000.0; rate_min=25, rate_max=90)
    @test collect(rates) ≈ ref["zoom_rates"]
    @test_throws BoundsError calculate_autocorrelation(ones(Float32, 100), 1000.0, 0, 0.5)   # Autocorrelations.jl:33
    # spectra
    _, y = getSpectrum(1.0, inp["sp_x"]; N=1000)
    @test maximum(abs.(y .- ref["sp_db"])) < 2e-3
    _, w = getWelch(1.0, inp["sp_x"]; sizeFFT=256)
    @test maximum(abs.(w .- ref["welch_db"])) < 1e-3
    _, _, m = getWaterfall(1.0, inp["sp_x"]; sizeFFT=128)
    @test eltype(m) == Float64 && size(m) == (128, 15)
    @test relmax(sqrt.(m), sqrt.(ref["wf"])) < 2e-5
    # fused loop body: the library's default mode is TSDR_FAST -> indices equal up to exact ties, pixels within 6e-7
    for tag in ("A", "B")
        g = inp["fr$(tag)_geom"]; S, y_t, x_t = Int(g[1]), Int(g[2]), Int(g[3])
        state = zeros(Float32, 600, 800)
        frames, sidx = hip_frames!(state, inp["fr$(tag)_iq"], SyncXY(state), S, y_t, x_t, 0.1f0)
        @test size(frames, 3) == Int(g[4])
        @test Int.(permutedims(sidx)) == Int.(ref["fr$(tag)_idx"])
        @test relmax(vec(state)[1:499:end], ref["fr$(tag)_state_sub"]) < 6e-7
    end
    # coherent stacking across buffers: a constant sample folds to itself; the lock turns a buffer that arrives a quarter turn off
    # back onto the state, the given phase does not
    let z0 = ComplexF32(0.3, -0.4), T = 40.5, F = 12, iq = fill(ComplexF32(0.3, -0.4), 600)
        zs = zeros(ComplexF32, 4, 4); mag = zeros(Float32, 4, 4)
        info = TempestHIP.hip_cstack!(zs, iq, 0.0, T, 0.0, 0.0, F; mag = mag)
        @test all(abs.(zs .- z0) .<= 1f-6) && all(abs.(mag .- 0.5f0) .<= 1f-6) && info[1] == 0.0 && info[7] == 1.0
        info = TempestHIP.hip_cstack!(zs, iq, 0.0, T, 0.0, 0.25, F; α = 0.5f0, mode = :lock, mag = mag)
        @test abs(info[5] + 0.25) <= 1e-6 && abs(info[6] - 1.0) <= 1e-6 && all(abs.(zs .- z0) .<= 1f-6)
        TempestHIP.hip_cstack!(zs, iq, 0.0, T, 0.0, 0.5, F; α = 0.5f0, mag = mag)
        @test all(mag .<= 1f-6)
        @test TempestHIP.cstack_plan(600, 0.0, T, 0.125, 0.5) == (14, 15 * T - 600, 0.375)
    end
    # carrier tracking: a constant sample probed along a track that turns frame f by 0.003 f^2 turns (0.36 at the last frame) shows
    # exactly those phases, the fit finds the quadratic (a_f + p(f) - p'(f)/2 = 0.003 f), and the stack along the zero track is the mean
    let z0 = ComplexF32(0.3, -0.4), T = 40.5, F = 12, iq = fill(ComplexF32(0.3, -0.4), 600)
        zref = fill(z0, 4, 4)
        track = TempestHIP.constant_track(F, 0.0)
        track[1, :] .= [0.003 * f^2 for f in 0:F-1]
        ρ, E_f, γ, E_s = TempestHIP.hip_ctrack_probe(iq, 0.0, T, track, F, zref)
        @test all(abs.(γ .- 1.0) .<= 1e-6) && abs(E_s - 16 * 0.25) <= 1e-5
        @test all(abs.(angle.(ρ) ./ 2π .+ [0.003 * f^2 for f in 0:F-1]) .<= 1e-6)
        fitted, coef = TempestHIP.fit_track(ρ, track)
        @test abs(coef[3] + 0.003) <= 1e-6 && all(abs.(fitted[1, :] .- 0.003 .* (0:F-1)) .<= 1e-5)
        zs = zeros(ComplexF32, 4, 4)
        TempestHIP.hip_ctrack_stack!(zs, iq, 0.0, T, TempestHIP.constant_track(F, 0.0), F)
        @test all(abs.(zs .- z0) .<= 1f-6)
    end
    # the frame Gram matrix: a constant sample turned by 0.003 f^2 turns gives G[f, g] = P |z0|^2 exp(-2πi (a_f - a_g)); the blind phases
    # are the track's, negated; the energy at those turns is the whole energy P |z0|^2
    let z0 = ComplexF32(0.3, -0.4), T = 40.5, F = 12, iq = fill(ComplexF32(0.3, -0.4), 600)
        a = [0.003 * f^2 for f in 0:F-1]
        track = TempestHIP.constant_track(F, 0.0)
        track[1, :] .= a
        G = TempestHIP.hip_ctrack_gram(iq, 0.0, T, track, F, 4, 4)
        @test all(abs.(G .- 16 * 0.25 .* [cispi(-2 * (a[f] - a[g])) for f in 1:F, g in 1:F]) .<= 1e-4)
        @test all(imag.(G[f, f]) == 0 for f in 1:F) && G == G'
        v, ρ = TempestHIP.gram_phases(G)
        @test all(abs.(v .- [cispi(-2 * x) for x in a]) .<= 1e-5)
        @test abs(TempestHIP.gram_energy(G, -a) - 4.0) <= 1e-4
        κ, e = TempestHIP.gram_carrier(TempestHIP.hip_ctrack_gram(iq, 0.0, T, nothing, F, 4, 4))
        @test min(κ, 1 - κ) <= 1e-6 && abs(e - 4.0) <= 1e-4
    end
    # the tuner: a tone at +0.125 Fs shifted by -0.125 Fs is the constant it started from, whatever unit-gain low-pass follows; two
    # chained calls give the bits of one
    let n = 4000, L = 31, D = 4, x = ComplexF32[0.5f0 * cispi(2 * 0.125 * m) for m in 0:n-1]
        h = TempestHIP.design_lowpass(L, D)
        ν = TempestHIP.freq_fix(-0.125, 1.0)
        @test ν == UInt64(7) << 61 && abs(sum(Float64.(h)) - 1) <= 1e-6 && h == reverse(h)
        cap, nxt = TempestHIP.tune_plan(0, n, L, D, 0, 0)
        y, hist = zeros(ComplexF32, cap), zeros(ComplexF32, L - 1)
        @test TempestHIP.hip_tune!(y, hist, x, 0, ν, UInt64(0), h, D, 0, 0) == cap == div(n - L, D) + 1
        @test all(abs.(y .- 0.5f0) .<= 1f-5)
        c1, n1 = TempestHIP.tune_plan(0, 1001, L, D, 0, 0)
        y2, h2 = zeros(ComplexF32, cap), zeros(ComplexF32, L - 1)
        @test TempestHIP.hip_tune!(y2, h2, x[1:1001], 0, ν, UInt64(0), h, D, 0, 0) == c1
        rest = zeros(ComplexF32, cap - c1)
        @test TempestHIP.hip_tune!(rest, h2, x[1002:end], n1.m0, ν, UInt64(0), h, D, n1.j0, n1.n_hist) == cap - c1
        @test vcat(y2[1:c1], rest) == y && h2 == hist
    end
end
