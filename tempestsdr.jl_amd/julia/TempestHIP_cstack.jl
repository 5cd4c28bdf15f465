# TempestHIP_cstack.jl -- part of module TempestHIP (included at its end, after TempestHIP_cfold.jl): the `ccall`s of
# include/tempest_hip_cstack.h, coherent stacking across buffers.  `hip_cfold!` keeps `abs(Z)` of a buffer and averages magnitudes
# across buffers; these functions keep the complex picture `Z`, turn it onto a complex state (by the caller's carried phase, or by the
# measured inner product of `Z` and the state: the phase lock) and blend the two as complex numbers: the magnitude is taken once, of
# the blended state.

const CSTACK_MODES = Dict(:given => Cint(0), :lock => Cint(1))   # TSDR_CSTACK_GIVEN, TSDR_CSTACK_LOCK

"""
    cstack_plan(n, t0, T, κ, φ; θ = 0.0) -> (F, next_t0, next_φ)

`F, next_t0 = fold_plan(n, t0, T)`; the frame that straddles the buffer's end is skipped but advances the carrier too:
`next_φ = frac(φ + θ + (F + 1) * κ)`, all in turns (`θ`: a measured residual, `info[5]` of a call, folded into the carried phase).
`t0 >= n`: `(0, t0 - n, φ)`.
"""
function cstack_plan(n::Integer, t0::Real, T::Real, κ::Real, φ::Real; θ::Real = 0.0)
    F, nt0 = fold_plan(n, t0, T)
    Float64(t0) >= Float64(n) && return 0, nt0, Float64(φ)
    x = Float64(φ) + Float64(θ) + (F + 1) * Float64(κ)
    return F, nt0, x - floor(x)
end

"""
    hip_cstack!(zstate, iq, t0, T, κ, φ, F; α = 0f0, mode = :given, mag = nothing) -> info

`zstate` (`y_t x x_t` `ComplexF32`) `<- α * zstate + (1 - α) * conj(q) * Z`, `Z` the complex mean of the `F` frames of period `T` from
`t0` in `iq`, frame `f` turned by `-(φ + f * κ)` turns; `q = 1` (`:given`) or `ρ / |ρ|`, `ρ = sum(Z .* conj.(zstate))` (`:lock`).
`mag` (`Matrix{Float32}`, optional) `<- abs.(zstate)`.  Returns the eight doubles `Re ρ, Im ρ, E_z, E_s, θ, γ, q`.  `α == 0`: the
state is overwritten without being read (`tsdr_cstack_iq`).
"""
function hip_cstack!(zstate::Matrix{ComplexF32}, iq::Vector{ComplexF32}, t0::Real, T::Real, κ::Real, φ::Real, F::Integer; α::Real = 0f0,
                     mode::Symbol = :given, mag::Union{Nothing, Matrix{Float32}} = nothing)
    haskey(CSTACK_MODES, mode) || throw(ArgumentError("unknown stacking mode $mode (:given, :lock)"))
    y_t, x_t = size(zstate)
    mag === nothing || size(mag) == (y_t, x_t) || throw(DimensionMismatch("mag must have the state's size"))
    info = zeros(Float64, 8)
    c = ctx()
    check(c, ccall((:tsdr_cstack_iq, LIB), Cint,
                   (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Cfloat, Csize_t, Cdouble, Cdouble, Cdouble, Cdouble, Cint, Cint, Cint, Cfloat, Cint,
                    Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float64}),
                   c.h, iq, IQ_FORMATS[:cf32], 1f0, length(iq), t0, T, κ, φ, F, y_t, x_t, α, CSTACK_MODES[mode], zstate,
                   mag === nothing ? C_NULL : pointer(mag), info), "hip_cstack!")
    return info
end

"""
    hip_cstack_d!(d_zstate, d_iq, fmt, scale, n, t0, T, κ, φ, F, y_t, x_t; α = 0f0, mode = :given, d_mag = C_NULL, d_info = C_NULL)

The same on device pointers (`d_iq`: `n` samples of format `fmt`, e.g. a raw ring slot; `d_mag`, `d_info` optional): enqueue-only on
the task's context (`tsdr_cstack_iq_d`).
"""
function hip_cstack_d!(d_zstate::Ptr{Cvoid}, d_iq::Ptr{Cvoid}, fmt::Symbol, scale::Real, n::Integer, t0::Real, T::Real, κ::Real, φ::Real,
                       F::Integer, y_t::Integer, x_t::Integer; α::Real = 0f0, mode::Symbol = :given, d_mag::Ptr{Cvoid} = C_NULL,
                       d_info::Ptr{Cvoid} = C_NULL)
    haskey(IQ_FORMATS, fmt) || throw(ArgumentError("unknown IQ format $fmt (:cf32, :sc16, :sc8, :uc8)"))
    haskey(CSTACK_MODES, mode) || throw(ArgumentError("unknown stacking mode $mode (:given, :lock)"))
    c = ctx()
    check(c, ccall((:tsdr_cstack_iq_d, LIB), Cint,
                   (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Cfloat, Csize_t, Cdouble, Cdouble, Cdouble, Cdouble, Cint, Cint, Cint, Cfloat, Cint,
                    Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
                   c.h, d_iq, IQ_FORMATS[fmt], scale, n, t0, T, κ, φ, F, y_t, x_t, α, CSTACK_MODES[mode], d_zstate, d_mag, d_info),
          "hip_cstack_d!")
    return nothing
end
