# TempestHIP_gram.jl -- part of module TempestHIP (included at its end, after TempestHIP_ctrack.jl): the `ccall`s of
# include/tempest_hip_gram.h, the Gram matrix of a buffer's frames, `G[f, g] = sum(v_f .* conj.(v_g))` along a track, and the host
# algorithms that read it: `gram_energy` (the energy of the coherent fold for any per-frame turns), `gram_carrier` (the maximum of the
# whole κ periodogram), `gram_phases` / `gram_track` (every frame's carrier phase with no reference picture), `track_slopes`,
# `blind_track`.  A track is a `2 x F` `Matrix{Float64}` as in TempestHIP_ctrack.jl.
# (This file is checked against the header's prototypes statically, tests/test_gram_host.py; it has not been run under Julia.)
import LinearAlgebra

const GRAM_MAX_FRAMES = 64

"""
    hip_ctrack_gram(iq, t0, T, track, F, y_t, x_t) -> F x F Matrix{ComplexF64}

`G[f + 1, g + 1] = sum_m v_f(m) * conj(v_g(m))`, the frames of `iq` turned along `track` (`nothing`: the zero track)
(`tsdr_ctrack_gram_iq`).
"""
function hip_ctrack_gram(iq::Vector{ComplexF32}, t0::Real, T::Real, track::Union{Nothing, Matrix{Float64}}, F::Integer, y_t::Integer,
                         x_t::Integer)
    track === nothing || size(track) == (2, F) || throw(DimensionMismatch("track must be 2 x $F"))
    out = zeros(Float64, 2 * F * F + 2)
    c = ctx()
    check(c, ccall((:tsdr_ctrack_gram_iq, LIB), Cint,
                   (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Cfloat, Csize_t, Cdouble, Cdouble, Ptr{Float64}, Cint, Cint, Cint, Ptr{Float64}),
                   c.h, iq, IQ_FORMATS[:cf32], 1f0, length(iq), t0, T, track === nothing ? C_NULL : pointer(track), F, y_t, x_t, out),
          "hip_ctrack_gram")
    rec = reshape(view(out, 1:2 * F * F), 2, F, F)          # (re / im, g, f): the library's rows are f
    return ComplexF64[complex(rec[1, g, f], rec[2, g, f]) for f in 1:F, g in 1:F]
end

"""
    hip_ctrack_gram_d!(d_gram, d_iq, fmt, scale, n, t0, T, d_track, F, y_t, x_t)

The same on device pointers (`d_gram`: `2 F^2` doubles, row-major (re, im) pairs; `d_track` may be `C_NULL`): enqueue-only
(`tsdr_ctrack_gram_iq_d`).
"""
function hip_ctrack_gram_d!(d_gram::Ptr{Cvoid}, d_iq::Ptr{Cvoid}, fmt::Symbol, scale::Real, n::Integer, t0::Real, T::Real,
                            d_track::Ptr{Cvoid}, F::Integer, y_t::Integer, x_t::Integer)
    haskey(IQ_FORMATS, fmt) || throw(ArgumentError("unknown IQ format $fmt (:cf32, :sc16, :sc8, :uc8)"))
    c = ctx()
    check(c, ccall((:tsdr_ctrack_gram_iq_d, LIB), Cint,
                   (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Cfloat, Csize_t, Cdouble, Cdouble, Ptr{Cvoid}, Cint, Cint, Cint, Ptr{Cvoid}),
                   c.h, d_iq, IQ_FORMATS[fmt], scale, n, t0, T, d_track, F, y_t, x_t, d_gram), "hip_ctrack_gram_d!")
    return nothing
end

"""
    gram_energy(G, turns) -> Float64

The energy of the coherent fold `Z = (1/F) sum_f exp(-2πi a_f) v_f` for per-frame turns `a_f = turns[f + 1]`, from `G` alone.
"""
function gram_energy(G::AbstractMatrix{<:Complex}, turns::AbstractVector{<:Real})
    F = length(turns)
    size(G) == (F, F) || throw(DimensionMismatch("G must be $F x $F"))
    w = [cispi(-2 * (a - floor(a))) for a in turns]
    return real(transpose(w) * G * conj.(w)) / F^2
end

"""
    gram_carrier(G; oversample = 16, steps = 4) -> (κ, energy)

The maximum of the κ periodogram of `G`: the lag sums `R(d) = sum_f G[f + d, f]`, the energy on `oversample * F` grid points, its
first maximum, then `steps` Newton steps on the energy's derivative, each kept inside one grid step.
"""
function gram_carrier(G::AbstractMatrix{<:Complex}; oversample::Integer = 16, steps::Integer = 4)
    F = size(G, 1)
    R = [sum(G[f + d, f] for f in 1:F-d) for d in 0:F-1]
    energy(k, order) = ((order == 0 ? real(R[1]) : 0.0) +
                        2 * real(sum((-2π * im * d)^order * cispi(-2 * d * k) * R[d + 1] for d in 1:F-1; init = 0.0 + 0.0im))) / F^2
    F == 1 && return 0.0, energy(0.0, 0)
    n = oversample * F
    h = 1.0 / n
    k = (argmax([energy(j * h, 0) for j in 0:n-1]) - 1) * h
    for _ in 1:steps
        e1, e2 = energy(k, 1), energy(k, 2)
        e2 < 0 || break
        k += clamp(-e1 / e2, -h, h)
    end
    return mod(k, 1.0), energy(k, 0)
end

"""
    gram_phases(G; iters = 50) -> (v, ρ)

`v_f` of unit modulus with `v[1] == 1`, the carrier phase of every frame; `ρ = G0 * v`, `G0 = G` with a zero diagonal.  `v` starts as
the eigenvector of `G0`'s largest eigenvalue scaled entrywise to unit modulus, then `r = G0 * v`, `v .= r ./ abs.(r)`.
"""
function gram_phases(G::AbstractMatrix{<:Complex}; iters::Integer = 50)
    F = size(G, 1)
    G0 = Matrix{ComplexF64}(G)
    for f in 1:F
        G0[f, f] = 0
    end
    F == 1 && return ones(ComplexF64, 1), zeros(ComplexF64, 1)
    v = LinearAlgebra.eigen(LinearAlgebra.Hermitian((G0 + G0') / 2)).vectors[:, end]
    v = [abs(x) > 0 ? x / abs(x) : one(ComplexF64) for x in v]
    for _ in 1:iters
        r = G0 * v
        nv = [abs(r[f]) > 0 ? r[f] / abs(r[f]) : v[f] for f in 1:F]
        done = maximum(abs.(nv .- v)) <= 1e-12
        v = nv
        done && break
    end
    v = v .* conj(v[1])
    v[1] = 1
    return v, G0 * v
end

"""
    gram_track(G; track = nothing) -> track

`track` (the one `G` was measured along; `nothing`: zeros) with `a_f += angle(v_f) / 2π`.
"""
function gram_track(G::AbstractMatrix{<:Complex}; track::Union{Nothing, Matrix{Float64}} = nothing)
    F = size(G, 1)
    t = track === nothing ? zeros(Float64, 2, F) : copy(track)
    t[1, :] .+= angle.(gram_phases(G)[1]) ./ 2π
    return t
end

"""
    track_slopes(track) -> track

`d_f = a_{f+1} - a_f`, `d_0` moved into `[-1/2, 1/2)` and every later one to lie nearest its predecessor; `b_f` = the mean of
`d_{f-1}` and `d_f` (one-sided at the ends); `a_f -= b_f / 2`.
"""
function track_slopes(track::Matrix{Float64})
    t = copy(track)
    F = size(t, 2)
    if F < 2
        t[2, :] .= 0
        return t
    end
    d = diff(t[1, :])
    d[1] -= floor(d[1] + 0.5)
    for f in 2:F-1
        d[f] += round(d[f - 1] - d[f])
    end
    for f in 1:F
        b = f == 1 ? d[1] : f == F ? d[end] : (d[f - 1] + d[f]) / 2
        t[2, f] = b
        t[1, f] -= b / 2
    end
    return t
end

"""
    blind_track(iq, t0, T, F, y_t, x_t; passes = 2) -> (track, abs.(ρ), zstate)

The carrier's phase track of one buffer with no start κ and no reference picture (host arrays): the Gram matrix with no track,
`gram_track`, `track_slopes`; per further pass the Gram matrix along the slope-only track; then `hip_ctrack_stack!` along the track.
"""
function blind_track(iq::Vector{ComplexF32}, t0::Real, T::Real, F::Integer, y_t::Integer, x_t::Integer; passes::Integer = 2)
    1 <= F <= GRAM_MAX_FRAMES || throw(ArgumentError("F must be in 1:$GRAM_MAX_FRAMES"))
    G = hip_ctrack_gram(iq, t0, T, nothing, F, y_t, x_t)
    track, ρ = track_slopes(gram_track(G)), gram_phases(G)[2]
    for k in 2:passes
        k > 2 && (track = track_slopes(vcat(transpose(track[1, :] .+ track[2, :] ./ 2), zeros(1, F))))
        slopes = vcat(zeros(1, F), transpose(track[2, :]))
        G = hip_ctrack_gram(iq, t0, T, slopes, F, y_t, x_t)
        track, ρ = gram_track(G; track = slopes), gram_phases(G)[2]
    end
    zs = zeros(ComplexF32, y_t, x_t)
    hip_ctrack_stack!(zs, iq, t0, T, track, F)
    return track, abs.(ρ), zs
end
