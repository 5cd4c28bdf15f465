# TempestHIP_cfold.jl -- part of module TempestHIP (included at its end, after TempestHIP_fold.jl): the `ccall`s of
# include/tempest_hip_cfold.h, phase-coherent frame folding with carrier de-rotation.  `hip_fold!` folds `abs.(iq)`; these functions
# fold the complex samples themselves: frame `f` is turned by `-f * κ` turns (`κ = frac(ν * T)`, the carrier's advance per frame),
# the frames are summed, and the magnitude is taken once at the end -- the noise averages down before the detector, not after it.

"""
    hip_cfold!(state, iq, t0, T, κ, F; α = 0f0) -> state

`state` (`y_t x x_t` `Float32`) `<- α * state + (1 - α) * abs(mean over f of exp(-2πi f κ) * frame f)`, the `F` frames of period `T`
(samples, fractional) that start at `t0` in `iq`, each sampled at `t0 + f*T + ((m + 1/2) * T/P - 1/2)` with linear interpolation of
`iq`.  `α == 0`: the state is overwritten without being read (`tsdr_cfold_iq`).
"""
function hip_cfold!(state::Matrix{Float32}, iq::Vector{ComplexF32}, t0::Real, T::Real, κ::Real, F::Integer; α::Real = 0f0)
    y_t, x_t = size(state)
    c = ctx()
    check(c, ccall((:tsdr_cfold_iq, LIB), Cint,
                   (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Cfloat, Csize_t, Cdouble, Cdouble, Cdouble, Cint, Cint, Cint, Cfloat, Ptr{Float32}),
                   c.h, iq, IQ_FORMATS[:cf32], 1f0, length(iq), t0, T, κ, F, y_t, x_t, α, state), "hip_cfold!")
    return state
end

"""
    hip_cfold_d!(d_state, d_iq, fmt, scale, n, t0, T, κ, F, y_t, x_t; α = 0f0)

The same on device pointers (`d_iq`: `n` samples of format `fmt`, e.g. a raw ring slot): enqueue-only on the task's context
(`tsdr_cfold_iq_d`).
"""
function hip_cfold_d!(d_state::Ptr{Cvoid}, d_iq::Ptr{Cvoid}, fmt::Symbol, scale::Real, n::Integer, t0::Real, T::Real, κ::Real,
                      F::Integer, y_t::Integer, x_t::Integer; α::Real = 0f0)
    haskey(IQ_FORMATS, fmt) || throw(ArgumentError("unknown IQ format $fmt (:cf32, :sc16, :sc8, :uc8)"))
    c = ctx()
    check(c, ccall((:tsdr_cfold_iq_d, LIB), Cint,
                   (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Cfloat, Csize_t, Cdouble, Cdouble, Cdouble, Cint, Cint, Cint, Cfloat, Ptr{Cvoid}),
                   c.h, d_iq, IQ_FORMATS[fmt], scale, n, t0, T, κ, F, y_t, x_t, α, d_state), "hip_cfold_d!")
    return nothing
end

"""
    hip_cfold_scan(iq, t0, T, κ0, dκ, n_trials, F, y_t, x_t) -> (scores, best)

`scores[k + 1]` = the energy of the complex picture folded at `κ0 + k * dκ`, all at the one period `T`; `best` = the one-based index
of the first maximum (`0` when every score is `NaN`) (`tsdr_cfold_scan_iq`).
"""
function hip_cfold_scan(iq::Vector{ComplexF32}, t0::Real, T::Real, κ0::Real, dκ::Real, n_trials::Integer, F::Integer, y_t::Integer,
                        x_t::Integer)
    scores = zeros(Float64, n_trials)
    best = Ref{Cint}(-1)
    c = ctx()
    check(c, ccall((:tsdr_cfold_scan_iq, LIB), Cint,
                   (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Cfloat, Csize_t, Cdouble, Cdouble, Cdouble, Cdouble, Cint, Cint, Cint, Cint, Ptr{Float64},
                    Ptr{Cint}),
                   c.h, iq, IQ_FORMATS[:cf32], 1f0, length(iq), t0, T, κ0, dκ, n_trials, F, y_t, x_t, scores, best), "hip_cfold_scan")
    return scores, Int(best[]) + 1
end

"""
    hip_cfold_scan_d!(d_score, d_iq, fmt, scale, n, t0, T, κ0, dκ, n_trials, F, y_t, x_t)

The same on device pointers (`d_score`: `n_trials` `Float64`): enqueue-only (`tsdr_cfold_scan_iq_d`).
"""
function hip_cfold_scan_d!(d_score::Ptr{Cvoid}, d_iq::Ptr{Cvoid}, fmt::Symbol, scale::Real, n::Integer, t0::Real, T::Real, κ0::Real,
                           dκ::Real, n_trials::Integer, F::Integer, y_t::Integer, x_t::Integer)
    haskey(IQ_FORMATS, fmt) || throw(ArgumentError("unknown IQ format $fmt (:cf32, :sc16, :sc8, :uc8)"))
    c = ctx()
    check(c, ccall((:tsdr_cfold_scan_iq_d, LIB), Cint,
                   (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Cfloat, Csize_t, Cdouble, Cdouble, Cdouble, Cdouble, Cint, Cint, Cint, Cint, Ptr{Cvoid}),
                   c.h, d_iq, IQ_FORMATS[fmt], scale, n, t0, T, κ0, dκ, n_trials, F, y_t, x_t, d_score), "hip_cfold_scan_d!")
    return nothing
end

"""
    refine_carrier(iq, t0, T, F, y_t, x_t; oversample = 4, half = 8, levels = 2, shrink = 4) -> (κ̂, last_dκ, scores)

The carrier's advance per frame in turns, from nothing: level 0 scans `oversample * F` trials over `[0, 1)` at
`dκ = 1 / (oversample * F)`; each further level scans `2 * half + 1` trials around the first maximum at `dκ / shrink`.  Returns
`κ̂ mod 1`, the last step and one score vector per level.  A host loop over `hip_cfold_scan`; it names no symbol itself.
"""
function refine_carrier(iq::Vector{ComplexF32}, t0::Real, T::Real, F::Integer, y_t::Integer, x_t::Integer; oversample::Integer = 4,
                        half::Integer = 8, levels::Integer = 2, shrink::Real = 4)
    (F >= 1 && oversample >= 1 && levels >= 1) || throw(ArgumentError("refine_carrier: F, oversample and levels must be positive"))
    step = 1.0 / (oversample * F)
    κ0, count, last, κ̂ = 0.0, oversample * F, step, 0.0
    scores = Vector{Vector{Float64}}()
    for _ in 1:levels
        s, b = hip_cfold_scan(iq, t0, T, κ0, step, count, F, y_t, x_t)
        push!(scores, s)
        b >= 1 || throw(ErrorException("refine_carrier: every score is NaN"))
        κ̂, last = κ0 + (b - 1) * step, step
        step /= shrink
        κ0, count = κ̂ - half * step, 2 * half + 1
    end
    return mod(κ̂, 1.0), last, scores
end
