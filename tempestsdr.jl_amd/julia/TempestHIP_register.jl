# TempestHIP_register.jl -- part of module TempestHIP (included at its end, after TempestHIP_hires.jl): the `ccall`s of
# include/tempest_hip_register.h, registration of the full-size rasters to the raster pixel.  The frame loop's sync indices live on
# RENDERING_SIZE; one of its steps is several raster pixels.  `hip_raster_register!` refines such shifts by correlating column and
# row sums with those of a reference picture; `hip_frames_hires!` does the same per chunk once `hip_hires_refine!(k)` has set k > 0.

"""
    hip_raster_register!(shifts_out, rasters, d_y, d_x; ref = nothing, shifts = nothing, units = :raster, grid = RENDERING_SIZE,
                         scores = nothing) -> shifts_out

`shifts_out` (`2 x n` `Cint`, `[1, f] = r_y`, `[2, f] = r_x` in raster lines / pixels) receives, for every raster
`rasters[:, :, f]`, its coarse shift (`shifts`, a `2 x n` integer matrix in `units` as `hip_raster_accumulate!` takes it;
`nothing` = 0) moved by the `d` in `-d_y:d_y` / `-d_x:d_x` whose score `sum(ref_profile .* circshift(profile, -(r0 + d)))` is
largest, candidates visited in the order 0, -1, +1, -2, +2, ... and replaced on a strict `>` only.  Profiles are column / row sums
in Float64.  `ref` is a `y_t x x_t` picture (the running average); `nothing`, or a picture whose profile is flat, means the first
raster.  `scores`, when given, is a `(2 d_y + 1 + 2 d_x + 1) x n` `Float64` matrix (`tsdr_raster_register`).
"""
function hip_raster_register!(shifts_out::Matrix{Cint}, rasters::Array{Float32,3}, d_y::Integer, d_x::Integer; ref = nothing,
                              shifts = nothing, units::Symbol = :raster, grid = RENDERING_SIZE, scores = nothing)
    haskey(SHIFT_UNITS, units) || throw(ArgumentError("unknown shift units $units (:raster, :image)"))
    y_t, x_t, n = size(rasters)
    size(shifts_out) == (2, n) || throw(DimensionMismatch("shifts_out must be 2 x $n"))
    ref === nothing || (ref isa Matrix{Float32} && size(ref) == (y_t, x_t)) || throw(DimensionMismatch("ref does not match the rasters"))
    sh = shifts === nothing ? Cint[] : Matrix{Cint}(shifts)
    shifts === nothing || size(sh) == (2, n) || throw(DimensionMismatch("shifts must be 2 x $n"))
    scores === nothing || (scores isa Matrix{Float64} && size(scores) == (2 * d_y + 1 + 2 * d_x + 1, n)) ||
        throw(DimensionMismatch("scores must be $(2 * d_y + 1 + 2 * d_x + 1) x $n Float64"))
    c = ctx()
    check(c, ccall((:tsdr_raster_register, LIB), Cint,
                   (Ptr{Cvoid}, Ptr{Float32}, Cint, Cint, Cint, Ptr{Float32}, Ptr{Cint}, Cint, Cint, Cint, Cint, Cint, Ptr{Cint}, Ptr{Float64}),
                   c.h, rasters, n, y_t, x_t, ref === nothing ? C_NULL : ref, shifts === nothing ? C_NULL : sh, SHIFT_UNITS[units],
                   grid[1], grid[2], d_y, d_x, shifts_out, scores === nothing ? C_NULL : scores), "hip_raster_register!")
    return shifts_out
end

"""
    hip_hires_refine!(k)

Context option "hires_refine": `k = 0` (default) leaves `hip_frames_hires!` as it is; `k` in `1:8` makes it register every chunk's
rasters to the running full-size average within `k` cells of the sync grid before averaging them.
"""
hip_hires_refine!(k::Integer) = hip_set_option("hires_refine", k)
