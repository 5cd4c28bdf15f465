# TempestHIP_tune.jl -- part of module TempestHIP (included at its end, after TempestHIP_gram.jl): the `ccall`s of
# include/tempest_hip_tune.h, the tuner -- frequency shift by a 64-bit phase accumulator, real FIR low-pass, decimation, chained
# across calls -- and the host helpers around it: `freq_fix`, `design_lowpass`, `tune_plan`.
# (This file is checked against the header's prototypes statically, tests/test_tune_host.py; it has not been run under Julia.)

const TUNE_TAPS_MAX = 1024
const TUNE_DECIM_MAX = 64

"""
    freq_fix(f_hz, Fs) -> UInt64

`nu_fix` (turns * 2^64 per sample, wrapped) of a shift BY `f_hz` at sample rate `Fs`; bringing a carrier at `+f` to DC needs
`freq_fix(-f, Fs)`.  Exact rational arithmetic on the two floats, rounded once.
"""
function freq_fix(f_hz::Real, Fs::Real)
    isfinite(f_hz) && isfinite(Fs) && Fs > 0 || throw(ArgumentError("f_hz must be finite and Fs positive"))
    turns = rationalize(BigInt, Float64(f_hz); tol = 0) // rationalize(BigInt, Float64(Fs); tol = 0)
    return UInt64(mod(round(BigInt, turns * (big(1) << 64)), big(1) << 64))
end

"""
    design_lowpass(L, D; width = 0.9, window = :blackman) -> Vector{Float32}

A windowed sinc with cut-off `width / (2 D)` cycles per input sample, normalised to unit DC gain in Float64, then rounded.
"""
function design_lowpass(L::Integer, D::Integer; width::Real = 0.9, window::Symbol = :blackman)
    1 <= L <= TUNE_TAPS_MAX && 1 <= D <= TUNE_DECIM_MAX && 0 < width <= 1 || throw(ArgumentError("L, D or width out of range"))
    x = [L == 1 ? 0.0 : 2π * k / (L - 1) for k in 0:L-1]
    w = window == :blackman ? 0.42 .- 0.5 .* cos.(x) .+ 0.08 .* cos.(2 .* x) :
        window == :hamming ? 0.54 .- 0.46 .* cos.(x) :
        window == :hann ? 0.5 .- 0.5 .* cos.(x) :
        window == :rect ? ones(L) : throw(ArgumentError("unknown window $window (:blackman, :hamming, :hann, :rect)"))
    L == 1 && (w = ones(1))
    h = [sinc(width * (i - (L - 1) / 2) / D) for i in 0:L-1] .* w
    return Float32.(h ./ sum(h))
end

"""
    tune_plan(m0, n, L, D, j0, n_hist) -> (n_out, next)

The outputs a call writes, `j0 .. floor((m0 + n - L) / D)`, and the arguments of the call that follows it:
`next = (m0 = m0 + n, j0 = j0 + n_out, n_hist = min(L - 1, n_hist + n), decim = D, delay = (L - 1) / 2)`.
"""
function tune_plan(m0::Integer, n::Integer, L::Integer, D::Integer, j0::Integer, n_hist::Integer)
    1 <= L <= TUNE_TAPS_MAX && 1 <= D <= TUNE_DECIM_MAX && 0 <= n < 2^31 && 0 <= n_hist <= min(L - 1, m0) ||
        throw(ArgumentError("tune_plan: arguments out of range"))
    big(j0) * D >= big(m0) - n_hist || throw(ArgumentError("tune_plan: the window of j0 starts before the history"))
    stop = big(m0) + n
    n_out = stop >= L ? max(Int(div(stop - L, D) - j0 + 1), 0) : 0
    return n_out, (m0 = UInt64(stop), j0 = UInt64(j0 + n_out), n_hist = Int(min(L - 1, n_hist + n)), decim = Int(D), delay = (L - 1) / 2)
end

"""
    hip_tune!(out, hist, iq, m0, nu_fix, phi_fix, taps, D, j0, n_hist) -> n_out

Host arrays: `out[1:n_out]` <- `y[j0 ..]` of `iq` (`iq[1]` is `x[m0]`), `hist` (`length(taps) - 1` ComplexF32) carried forward
(`tsdr_tune_iq`).
"""
function hip_tune!(out::Vector{ComplexF32}, hist::Vector{ComplexF32}, iq::Vector{ComplexF32}, m0::Integer, nu_fix::UInt64,
                   phi_fix::UInt64, taps::Vector{Float32}, D::Integer, j0::Integer, n_hist::Integer)
    length(hist) >= length(taps) - 1 || throw(DimensionMismatch("hist must hold length(taps) - 1 samples"))
    n_out = Ref{Csize_t}(0)
    c = ctx()
    check(c, ccall((:tsdr_tune_iq, LIB), Cint,
                   (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Cfloat, Csize_t, UInt64, UInt64, UInt64, Ptr{Float32}, Cint, Cint, UInt64, Ptr{Cvoid}, Cint,
                    Ptr{Cvoid}, Csize_t, Ref{Csize_t}),
                   c.h, iq, IQ_FORMATS[:cf32], 1f0, length(iq), m0, nu_fix, phi_fix, taps, length(taps), D, j0, hist, n_hist, out,
                   length(out), n_out), "hip_tune!")
    return Int(n_out[])
end

"""
    hip_tune_d!(d_out, out_cap, d_hist, d_iq, fmt, scale, n, m0, nu_fix, phi_fix, d_taps, L, D, j0, n_hist) -> n_out

The same on device pointers (`d_hist` may be `C_NULL` with `n_hist == 0`): enqueue-only; `n_out` is computed on the host
(`tsdr_tune_iq_d`).
"""
function hip_tune_d!(d_out::Ptr{Cvoid}, out_cap::Integer, d_hist::Ptr{Cvoid}, d_iq::Ptr{Cvoid}, fmt::Symbol, scale::Real, n::Integer,
                     m0::Integer, nu_fix::UInt64, phi_fix::UInt64, d_taps::Ptr{Cvoid}, L::Integer, D::Integer, j0::Integer,
                     n_hist::Integer)
    haskey(IQ_FORMATS, fmt) || throw(ArgumentError("unknown IQ format $fmt (:cf32, :sc16, :sc8, :uc8)"))
    n_out = Ref{Csize_t}(0)
    c = ctx()
    check(c, ccall((:tsdr_tune_iq_d, LIB), Cint,
                   (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Cfloat, Csize_t, UInt64, UInt64, UInt64, Ptr{Cvoid}, Cint, Cint, UInt64, Ptr{Cvoid}, Cint,
                    Ptr{Cvoid}, Csize_t, Ref{Csize_t}),
                   c.h, d_iq, IQ_FORMATS[fmt], scale, n, m0, nu_fix, phi_fix, d_taps, L, D, j0, d_hist, n_hist, d_out, out_cap, n_out),
          "hip_tune_d!")
    return Int(n_out[])
end

"""
    tune_tile(L, D) -> outputs per workgroup of the kernel (`tsdr_tune_tile`)
"""
function tune_tile(L::Integer, D::Integer)
    r = ccall((:tsdr_tune_tile, LIB), Cint, (Cint, Cint), L, D)
    r > 0 || throw(ArgumentError("tune_tile: L or D out of range"))
    return Int(r)
end
