# TempestHIP_fold.jl -- part of module TempestHIP (included at its end, after TempestHIP_display.jl): the `ccall`s of
# include/tempest_hip_fold.h, coherent frame folding at a fractional frame period.  The reference cuts a buffer into frames of
# `round(Fs/fv)` samples (GUI.jl:103-109,137,166) and aligns each by its own `vsync`; these functions sample the frames at
# `t0 + f*T` with the true, fractional `T`, average them pixel by pixel, and score the pictures folded at trial periods.

"""
    fold_plan(n, t0, T) -> (F, next_t0)

`F = floor((n - t0) / T)` frames of period `T` fit a buffer of `n` samples whose first whole frame starts at `t0`; the frame that
straddles the end is skipped and the phase kept: `next_t0 = t0 + (F + 1) * T - n`, in `(0, T]`.  (`t0 >= n`: no frame starts in this
buffer, `(0, t0 - n)`.)
"""
function fold_plan(n::Integer, t0::Real, T::Real)
    n64, t, p = Float64(n), Float64(t0), Float64(T)
    (p > 0 && t >= 0) || throw(ArgumentError("fold_plan: T must be positive and t0 not negative"))
    t >= n64 && return 0, t - n64
    F = max(floor(Int, (n64 - t) / p), 0)
    while F > 0 && t + F * p > n64
        F -= 1
    end
    while t + (F + 1) * p <= n64
        F += 1
    end
    return F, t + (F + 1) * p - n64
end

"""
    hip_fold!(state, iq, t0, T, F; α = 0f0) -> state

`state` (`y_t x x_t` `Float32`) `<- α * state + (1 - α) *` the mean of the `F` frames of period `T` (samples, fractional) that start at
`t0` in `iq`, each sampled at `t0 + f*T + ((m + 1/2) * T/P - 1/2)` with linear interpolation of `abs.(iq)`.  `α == 0`: the state is
overwritten without being read (`tsdr_fold_iq`).
"""
function hip_fold!(state::Matrix{Float32}, iq::Vector{ComplexF32}, t0::Real, T::Real, F::Integer; α::Real = 0f0)
    y_t, x_t = size(state)
    c = ctx()
    check(c, ccall((:tsdr_fold_iq, LIB), Cint,
                   (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Cfloat, Csize_t, Cdouble, Cdouble, Cint, Cint, Cint, Cfloat, Ptr{Float32}),
                   c.h, iq, IQ_FORMATS[:cf32], 1f0, length(iq), t0, T, F, y_t, x_t, α, state), "hip_fold!")
    return state
end

"""
    hip_fold_d!(d_state, d_iq, fmt, scale, n, t0, T, F, y_t, x_t; α = 0f0)

The same on device pointers (`d_iq`: `n` samples of format `fmt`, e.g. a raw ring slot): enqueue-only on the task's context
(`tsdr_fold_iq_d`).
"""
function hip_fold_d!(d_state::Ptr{Cvoid}, d_iq::Ptr{Cvoid}, fmt::Symbol, scale::Real, n::Integer, t0::Real, T::Real, F::Integer,
                     y_t::Integer, x_t::Integer; α::Real = 0f0)
    haskey(IQ_FORMATS, fmt) || throw(ArgumentError("unknown IQ format $fmt (:cf32, :sc16, :sc8, :uc8)"))
    c = ctx()
    check(c, ccall((:tsdr_fold_iq_d, LIB), Cint,
                   (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Cfloat, Csize_t, Cdouble, Cdouble, Cint, Cint, Cint, Cfloat, Ptr{Cvoid}),
                   c.h, d_iq, IQ_FORMATS[fmt], scale, n, t0, T, F, y_t, x_t, α, d_state), "hip_fold_d!")
    return nothing
end

"""
    hip_fold_scan(iq, t0, T0, dT, n_trials, F, y_t, x_t) -> (scores, best)

`scores[k + 1]` = the variance times `y_t * x_t` of the picture folded at `T0 + k * dT`; `best` = the one-based index of the first
maximum (`0` when every score is `NaN`) (`tsdr_fold_scan_iq`).
"""
function hip_fold_scan(iq::Vector{ComplexF32}, t0::Real, T0::Real, dT::Real, n_trials::Integer, F::Integer, y_t::Integer, x_t::Integer)
    scores = zeros(Float64, n_trials)
    best = Ref{Cint}(-1)
    c = ctx()
    check(c, ccall((:tsdr_fold_scan_iq, LIB), Cint,
                   (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Cfloat, Csize_t, Cdouble, Cdouble, Cdouble, Cint, Cint, Cint, Cint, Ptr{Float64}, Ptr{Cint}),
                   c.h, iq, IQ_FORMATS[:cf32], 1f0, length(iq), t0, T0, dT, n_trials, F, y_t, x_t, scores, best), "hip_fold_scan")
    return scores, Int(best[]) + 1
end

"""
    hip_fold_scan_d!(d_score, d_iq, fmt, scale, n, t0, T0, dT, n_trials, F, y_t, x_t)

The same on device pointers (`d_score`: `n_trials` `Float64`): enqueue-only (`tsdr_fold_scan_iq_d`).
"""
function hip_fold_scan_d!(d_score::Ptr{Cvoid}, d_iq::Ptr{Cvoid}, fmt::Symbol, scale::Real, n::Integer, t0::Real, T0::Real, dT::Real,
                          n_trials::Integer, F::Integer, y_t::Integer, x_t::Integer)
    haskey(IQ_FORMATS, fmt) || throw(ArgumentError("unknown IQ format $fmt (:cf32, :sc16, :sc8, :uc8)"))
    c = ctx()
    check(c, ccall((:tsdr_fold_scan_iq_d, LIB), Cint,
                   (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Cfloat, Csize_t, Cdouble, Cdouble, Cdouble, Cint, Cint, Cint, Cint, Ptr{Cvoid}),
                   c.h, d_iq, IQ_FORMATS[fmt], scale, n, t0, T0, dT, n_trials, F, y_t, x_t, d_score), "hip_fold_scan_d!")
    return nothing
end
