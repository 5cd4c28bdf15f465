# TempestHIP_ctrack.jl -- part of module TempestHIP (included at its end, after TempestHIP_cstack.jl): the `ccall`s of
# include/tempest_hip_ctrack.h, carrier tracking.  `hip_cstack!` turns frame `f` by `φ + f * κ` turns, one constant advance per call
# and the same phase on every line; here the weight of a sample is a function of frame and raster line, given as data: a track of
# `(a_f, b_f)` turns per frame, a `2 x F` `Matrix{Float64}` (column `f + 1` is frame `f`).  `hip_ctrack_stack!` stacks along a track,
# `hip_ctrack_probe` measures every frame's phase against a picture; `fit_track` and `constant_track` are the host side of the loop.
# (This file is checked against the header's prototypes statically, tests/test_ctrack_host.py; it has not been run under Julia.)

"""
    constant_track(F, κ; φ = 0.0, slope = 0.0) -> 2 x F Matrix{Float64}

`a_f = f * κ + φ` (two roundings, as `hip_cstack!` forms its weights: with `slope == 0` the two agree bit for bit), `b_f = slope`.
"""
function constant_track(F::Integer, κ::Real; φ::Real = 0.0, slope::Real = 0.0)
    t = Matrix{Float64}(undef, 2, F)
    for f in 0:F-1
        x = Float64(f) * Float64(κ)
        t[1, f + 1] = x + Float64(φ)
        t[2, f + 1] = Float64(slope)
    end
    return t
end

"""
    fit_track(ρ, track; degree = 2) -> (track, coefficients)

`r_f = angle(ρ_f) / 2π`, unwrapped so that each value lies nearest to its predecessor (frames with `ρ_f == 0` are passed over); the
least-squares polynomial `p` of `degree` in `f` with weights `abs(ρ_f)`; `a_f += p(f) - p'(f) / 2`, `b_f += p'(f)`.  `coefficients[k + 1]`
belongs to `f^k`.
"""
function fit_track(ρ::AbstractVector{<:Complex}, track::Matrix{Float64}; degree::Integer = 2)
    F = length(ρ)
    size(track) == (2, F) || throw(DimensionMismatch("track must be 2 x $F"))
    t = copy(track)
    idx = [f for f in 0:F-1 if abs(ρ[f + 1]) > 0]
    isempty(idx) && return t, zeros(Float64, 1)
    r = Float64[]
    for f in idx
        x = angle(ρ[f + 1]) / (2π)
        isempty(r) || (x += round(r[end] - x))
        push!(r, x)
    end
    deg = max(0, min(degree, length(idx) - 1))
    w = sqrt.(abs.(ρ[idx .+ 1]))
    V = [w[i] * Float64(idx[i])^k for i in eachindex(idx), k in 0:deg]
    coef = V \ (w .* r)
    p(f) = sum(coef[k + 1] * f^k for k in 0:deg)
    dp(f) = sum(k * coef[k + 1] * f^(k - 1) for k in 1:deg; init = 0.0)
    for f in 0:F-1
        t[1, f + 1] += p(Float64(f)) - dp(Float64(f)) / 2
        t[2, f + 1] += dp(Float64(f))
    end
    return t, coef
end

"""
    hip_ctrack_stack!(zstate, iq, t0, T, track, F; α = 0f0, mode = :given, mag = nothing) -> info

`hip_cstack!` along `track`: frame `f` on line `l` is turned by `-(a_f + b_f * (l + 1/2) / y_t)` turns (`tsdr_ctrack_stack_iq`).
"""
function hip_ctrack_stack!(zstate::Matrix{ComplexF32}, iq::Vector{ComplexF32}, t0::Real, T::Real, track::Matrix{Float64}, F::Integer;
                           α::Real = 0f0, mode::Symbol = :given, mag::Union{Nothing, Matrix{Float32}} = nothing)
    haskey(CSTACK_MODES, mode) || throw(ArgumentError("unknown stacking mode $mode (:given, :lock)"))
    size(track) == (2, F) || throw(DimensionMismatch("track must be 2 x $F"))
    y_t, x_t = size(zstate)
    mag === nothing || size(mag) == (y_t, x_t) || throw(DimensionMismatch("mag must have the state's size"))
    info = zeros(Float64, 8)
    c = ctx()
    check(c, ccall((:tsdr_ctrack_stack_iq, LIB), Cint,
                   (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Cfloat, Csize_t, Cdouble, Cdouble, Ptr{Float64}, Cint, Cint, Cint, Cfloat, Cint,
                    Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float64}),
                   c.h, iq, IQ_FORMATS[:cf32], 1f0, length(iq), t0, T, track, F, y_t, x_t, α, CSTACK_MODES[mode], zstate,
                   mag === nothing ? C_NULL : pointer(mag), info), "hip_ctrack_stack!")
    return info
end

"""
    hip_ctrack_stack_d!(d_zstate, d_iq, fmt, scale, n, t0, T, d_track, F, y_t, x_t; α = 0f0, mode = :given, d_mag = C_NULL, d_info = C_NULL)

The same on device pointers (`d_track`: `2F` doubles on the device): enqueue-only on the task's context (`tsdr_ctrack_stack_iq_d`).
"""
function hip_ctrack_stack_d!(d_zstate::Ptr{Cvoid}, d_iq::Ptr{Cvoid}, fmt::Symbol, scale::Real, n::Integer, t0::Real, T::Real,
                             d_track::Ptr{Cvoid}, F::Integer, y_t::Integer, x_t::Integer; α::Real = 0f0, mode::Symbol = :given,
                             d_mag::Ptr{Cvoid} = C_NULL, d_info::Ptr{Cvoid} = C_NULL)
    haskey(IQ_FORMATS, fmt) || throw(ArgumentError("unknown IQ format $fmt (:cf32, :sc16, :sc8, :uc8)"))
    haskey(CSTACK_MODES, mode) || throw(ArgumentError("unknown stacking mode $mode (:given, :lock)"))
    c = ctx()
    check(c, ccall((:tsdr_ctrack_stack_iq_d, LIB), Cint,
                   (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Cfloat, Csize_t, Cdouble, Cdouble, Ptr{Cvoid}, Cint, Cint, Cint, Cfloat, Cint,
                    Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
                   c.h, d_iq, IQ_FORMATS[fmt], scale, n, t0, T, d_track, F, y_t, x_t, α, CSTACK_MODES[mode], d_zstate, d_mag, d_info),
          "hip_ctrack_stack_d!")
    return nothing
end

"""
    hip_ctrack_probe(iq, t0, T, track, F, zref) -> (ρ, E_f, γ, E_s)

Every frame's inner product with the picture `zref` (`y_t x x_t` `ComplexF32`) after the track's turn (`track === nothing`: the zero
track): `ρ_f = sum(w_f(l) * z_f .* conj.(zref))`, the frame's energy `E_f`, the coherence `γ_f`, and `E_s = sum(abs2, zref)`
(`tsdr_ctrack_probe_iq`).
"""
function hip_ctrack_probe(iq::Vector{ComplexF32}, t0::Real, T::Real, track::Union{Nothing, Matrix{Float64}}, F::Integer,
                          zref::Matrix{ComplexF32})
    track === nothing || size(track) == (2, F) || throw(DimensionMismatch("track must be 2 x $F"))
    y_t, x_t = size(zref)
    out = zeros(Float64, 4 * F + 1)
    c = ctx()
    check(c, ccall((:tsdr_ctrack_probe_iq, LIB), Cint,
                   (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Cfloat, Csize_t, Cdouble, Cdouble, Ptr{Float64}, Cint, Cint, Cint, Ptr{Cvoid}, Ptr{Float64}),
                   c.h, iq, IQ_FORMATS[:cf32], 1f0, length(iq), t0, T, track === nothing ? C_NULL : pointer(track), F, y_t, x_t, zref, out),
          "hip_ctrack_probe")
    rec = reshape(view(out, 1:4F), 4, F)
    return complex.(rec[1, :], rec[2, :]), rec[3, :], rec[4, :], out[4F + 1]
end

"""
    hip_ctrack_probe_d!(d_out, d_iq, fmt, scale, n, t0, T, d_track, F, y_t, x_t, d_zref)

The same on device pointers (`d_out`: `4F + 1` doubles; `d_track` may be `C_NULL`): enqueue-only (`tsdr_ctrack_probe_iq_d`).
"""
function hip_ctrack_probe_d!(d_out::Ptr{Cvoid}, d_iq::Ptr{Cvoid}, fmt::Symbol, scale::Real, n::Integer, t0::Real, T::Real,
                             d_track::Ptr{Cvoid}, F::Integer, y_t::Integer, x_t::Integer, d_zref::Ptr{Cvoid})
    haskey(IQ_FORMATS, fmt) || throw(ArgumentError("unknown IQ format $fmt (:cf32, :sc16, :sc8, :uc8)"))
    c = ctx()
    check(c, ccall((:tsdr_ctrack_probe_iq_d, LIB), Cint,
                   (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Cfloat, Csize_t, Cdouble, Cdouble, Ptr{Cvoid}, Cint, Cint, Cint, Ptr{Cvoid}, Ptr{Cvoid}),
                   c.h, d_iq, IQ_FORMATS[fmt], scale, n, t0, T, d_track, F, y_t, x_t, d_zref, d_out), "hip_ctrack_probe_d!")
    return nothing
end
