# TempestHIP_hires.jl -- part of module TempestHIP (included at its end): the `ccall`s of include/tempest_hip_hires.h, frame
# averaging at the monitor's own resolution.  The reference aligns and averages at RENDERING_SIZE only (GUI.jl:171-175 behind
# downgradeImage); these two functions run the same circshift + one-pole IIR on the y_t x x_t rasters.

const SHIFT_UNITS = Dict(:raster => 0, :image => 1)   # TSDR_SHIFT_*

"""
    hip_raster_accumulate!(state, rasters, α; shifts = nothing, units = :raster, grid = RENDERING_SIZE) -> state

`state .= α .* state .+ (1 - α) .* circshift(rasters[:, :, f], (-r_y, -r_x))` for every frame `f` in order, in Float32 with two
products and one sum (GUI.jl:172,175 at raster size).  `shifts` is a `2 x n` integer matrix (`[1, f] = s_y`, `[2, f] = s_x`, the
layout `hip_frames!` returns) in raster lines / pixels (`units = :raster`) or as indices of a `grid` sync image (`units = :image`:
`r_y = floor((2 s_y y_t + grid[1]) / (2 grid[1])) mod y_t`); `nothing` means no shift (`tsdr_raster_accum`).
"""
function hip_raster_accumulate!(state::Matrix{Float32}, rasters::Array{Float32,3}, α::Float32; shifts = nothing, units::Symbol = :raster,
                                grid = RENDERING_SIZE)
    haskey(SHIFT_UNITS, units) || throw(ArgumentError("unknown shift units $units (:raster, :image)"))
    y_t, x_t, n = size(rasters)
    size(state) == (y_t, x_t) || throw(DimensionMismatch("state does not match the rasters"))
    sh = shifts === nothing ? Cint[] : Matrix{Cint}(shifts)
    shifts === nothing || size(sh) == (2, n) || throw(DimensionMismatch("shifts must be 2 x $n"))
    c = ctx()
    check(c, ccall((:tsdr_raster_accum, LIB), Cint,
                   (Ptr{Cvoid}, Ptr{Float32}, Cint, Cint, Cint, Ptr{Cint}, Cint, Cint, Cint, Cfloat, Ptr{Float32}),
                   c.h, rasters, n, y_t, x_t, shifts === nothing ? C_NULL : sh, SHIFT_UNITS[units], grid[1], grid[2], α, state), "hip_raster_accumulate!")
    return state
end

"""
    hip_raster_accumulate_d!(d_state, d_rasters, n, y_t, x_t, α; d_shifts = C_NULL, units = :raster, grid = RENDERING_SIZE)

The same on device pointers: enqueue-only on the task's context (`tsdr_raster_accum_d`).
"""
function hip_raster_accumulate_d!(d_state::Ptr{Cvoid}, d_rasters::Ptr{Cvoid}, n::Integer, y_t, x_t, α::Float32; d_shifts::Ptr{Cvoid} = C_NULL,
                                  units::Symbol = :raster, grid = RENDERING_SIZE)
    haskey(SHIFT_UNITS, units) || throw(ArgumentError("unknown shift units $units (:raster, :image)"))
    c = ctx()
    check(c, ccall((:tsdr_raster_accum_d, LIB), Cint,
                   (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Cint, Cint, Ptr{Cvoid}, Cint, Cint, Cint, Cfloat, Ptr{Cvoid}),
                   c.h, d_rasters, n, y_t, x_t, d_shifts, SHIFT_UNITS[units], grid[1], grid[2], α, d_state), "hip_raster_accumulate_d!")
    return nothing
end

"""
    hip_frames_hires!(d_imageOut, d_hires, d_iq, fmt, scale, nEch, sync, S, y_t, x_t, α, α_hires; d_frames = C_NULL, d_idx = C_NULL, do_align = true) -> nb

The loop body of `hip_frames_submit_iq!` (one call per buffer, not pipelined) plus the full-size average: `d_hires` (`y_t x x_t`
Float32 on the device, in / out) receives the buffer's rasters, registered by the loop's own sync indices and averaged with
`α_hires`.  The buffer is walked in chunks (option "hires_chunk_frames"), so the raster workspace stays bounded
(`tsdr_frames_hires_iq_d`).
"""
function hip_frames_hires!(d_imageOut::Ptr{Cvoid}, d_hires::Ptr{Cvoid}, d_iq::Ptr{Cvoid}, fmt::Symbol, scale::Float32, nEch::Integer,
                           sync::SyncXY{Float32}, S, y_t, x_t, α::Float32, α_hires::Float32; d_frames::Ptr{Cvoid} = C_NULL,
                           d_idx::Ptr{Cvoid} = C_NULL, do_align = true)
    haskey(IQ_FORMATS, fmt) || throw(ArgumentError("unknown IQ format $fmt (:cf32, :sc16, :sc8, :uc8)"))
    n = Ref{Cint}(0)
    check(sync.c, ccall((:tsdr_frames_hires_iq_d, LIB), Cint,
                        (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Cint, Cfloat, Csize_t, Csize_t, Cint, Cint, Cfloat, Cint, Ptr{Cvoid}, Ptr{Cvoid}, Cfloat, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cint}),
                        sync.c.h, sync.h, d_iq, IQ_FORMATS[fmt], scale, nEch, S, y_t, x_t, α, do_align ? 1 : 0, d_imageOut, d_frames, α_hires, d_hires, d_idx, n), "hip_frames_hires!")
    return Int(n[])
end
