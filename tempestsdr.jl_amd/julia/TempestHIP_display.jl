# TempestHIP_display.jl -- part of module TempestHIP (included at its end, after TempestHIP_register.jl): the `ccall`s of
# include/tempest_hip_display.h, display export.  The reference normalises a picture on the host before showing it (`fullScale!`,
# ScreenRenderer.jl:35-39: `(mat .- min) / (max - min)`); these two functions crop a region of interest, stretch it over a fixed
# range, its finite minimum / maximum (`fullScale!` times 255) or two percentiles of it, and return bytes -- on the device.

const RANGE_MODES = Dict(:fixed => 0, :minmax => 1, :percentile => 2)   # TSDR_RANGE_*
display_flags(invert, shared) = Cint((invert ? 1 : 0) | (shared ? 2 : 0))   # TSDR_DISPLAY_INVERT | TSDR_DISPLAY_SHARED

"""
    hip_display_u8!(out, images; roi = nothing, mode = :minmax, lo = 0f0, hi = 1f0, p = (0.01, 0.99), invert = false, shared = false,
                    ranges = nothing) -> out

`out` (`rh x rw x n` `UInt8`) receives rows `i0 + 1 : i0 + rh`, columns `j0 + 1 : j0 + rw` of every picture `images[:, :, f]`
(`roi = (i0, j0, rh, rw)`, zero-based corner; `nothing` = the whole picture), mapped to `0:255` over `(lo, hi)` (`mode = :fixed`), the
ROI's finite minimum and maximum (`:minmax`), or the edges of the 4096-bin histogram bins holding the fractions `p` of its finite
pixels (`:percentile`).  `shared = true` uses one range for all pictures; `invert = true` gives `255 - q`.  `ranges`, when given,
is a `2 x n` `Float32` matrix that receives the `(lo, hi)` used (`tsdr_display_u8`).
"""
function hip_display_u8!(out::Array{UInt8,3}, images::Array{Float32,3}; roi = nothing, mode::Symbol = :minmax, lo::Real = 0f0, hi::Real = 1f0,
                         p = (0.01, 0.99), invert::Bool = false, shared::Bool = false, ranges = nothing)
    haskey(RANGE_MODES, mode) || throw(ArgumentError("unknown range mode $mode (:fixed, :minmax, :percentile)"))
    h, w, n = size(images)
    i0, j0, rh, rw = roi === nothing ? (0, 0, h, w) : roi
    size(out) == (rh, rw, n) || throw(DimensionMismatch("out must be $rh x $rw x $n"))
    ranges === nothing || (ranges isa Matrix{Float32} && size(ranges) == (2, n)) || throw(DimensionMismatch("ranges must be 2 x $n Float32"))
    c = ctx()
    check(c, ccall((:tsdr_display_u8, LIB), Cint,
                   (Ptr{Cvoid}, Ptr{Float32}, Cint, Cint, Cint, Cint, Cint, Cint, Cint, Cint, Cfloat, Cfloat, Cdouble, Cdouble, Cint, Ptr{UInt8}, Ptr{Float32}),
                   c.h, images, n, h, w, i0, j0, rh, rw, RANGE_MODES[mode], lo, hi, p[1], p[2], display_flags(invert, shared), out,
                   ranges === nothing ? C_NULL : ranges), "hip_display_u8!")
    return out
end

"""
    hip_display_u8_d!(d_out, d_images, n, h, w; roi = nothing, mode = :minmax, lo = 0f0, hi = 1f0, p = (0.01, 0.99), invert = false,
                      shared = false, d_ranges = C_NULL)

The same on device pointers: enqueue-only on the task's context.  `d_images` is what `hip_frames!`'s device forms leave
(`d_frames`, `d_imageOut`, `d_hires`); `d_out` may sit at any byte address (`tsdr_display_u8_d`).
"""
function hip_display_u8_d!(d_out::Ptr{Cvoid}, d_images::Ptr{Cvoid}, n::Integer, h::Integer, w::Integer; roi = nothing, mode::Symbol = :minmax,
                           lo::Real = 0f0, hi::Real = 1f0, p = (0.01, 0.99), invert::Bool = false, shared::Bool = false,
                           d_ranges::Ptr{Cvoid} = C_NULL)
    haskey(RANGE_MODES, mode) || throw(ArgumentError("unknown range mode $mode (:fixed, :minmax, :percentile)"))
    i0, j0, rh, rw = roi === nothing ? (0, 0, h, w) : roi
    c = ctx()
    check(c, ccall((:tsdr_display_u8_d, LIB), Cint,
                   (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Cint, Cint, Cint, Cint, Cint, Cint, Cint, Cfloat, Cfloat, Cdouble, Cdouble, Cint, Ptr{Cvoid}, Ptr{Cvoid}),
                   c.h, d_images, n, h, w, i0, j0, rh, rw, RANGE_MODES[mode], lo, hi, p[1], p[2], display_flags(invert, shared), d_out,
                   d_ranges), "hip_display_u8_d!")
    return nothing
end
