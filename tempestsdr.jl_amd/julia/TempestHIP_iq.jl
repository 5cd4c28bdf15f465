# TempestHIP_iq.jl -- part of module TempestHIP (included at its end): the `ccall`s of include/tempest_hip_iq.h, the device-pointer
# forms of the spectra and demodulators on integer IQ as the SDR stored it.

# Integer IQ (Complex{Int16} / Complex{Int8} / Complex{UInt8}, see getSpectrum in TempestHIP.jl): the device-pointer `_iq_d` entry points
# around an upload of the raw samples (2 or 4 bytes each); every component is (Float32(code) - offset) * scale in the kernel
function _demod_iq(sym_call, what, sig, scale::Float32)
    out = Vector{Float32}(undef, length(sig)); c = ctx()
    d_in = ccall((:tsdr_dev_alloc, LIB), Ptr{Cvoid}, (Ptr{Cvoid}, Csize_t), c.h, max(sizeof(sig), 8))
    d_out = ccall((:tsdr_dev_alloc, LIB), Ptr{Cvoid}, (Ptr{Cvoid}, Csize_t), c.h, max(sizeof(out), 8))
    (d_in == C_NULL || d_out == C_NULL) && throw(OutOfMemoryError())
    try
        check(c, ccall((:tsdr_upload, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Csize_t), c.h, d_in, sig, sizeof(sig)), "upload")
        check(c, sym_call(c, d_in, d_out), what)
        check(c, ccall((:tsdr_download, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Csize_t), c.h, out, d_out, sizeof(out)), "download")
    finally
        ccall((:tsdr_dev_free, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}), c.h, d_in)
        ccall((:tsdr_dev_free, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}), c.h, d_out)
    end
    return out
end
function amDemod(sig::Vector{<:Union{Complex{Int16},Complex{Int8},Complex{UInt8}}}; scale::Float32 = 1f0)
    code = _iq_code(sig); n = length(sig)
    _demod_iq("amDemod", sig, scale) do c, d_in, d_out
        ccall((:tsdr_am_demod_iq_d, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Cfloat, Csize_t, Ptr{Cvoid}), c.h, d_in, code, scale, n, d_out)
    end
end
function invert_amDemod(sig::Vector{<:Union{Complex{Int16},Complex{Int8},Complex{UInt8}}}; scale::Float32 = 1f0)
    code = _iq_code(sig); n = length(sig)
    _demod_iq("invert_amDemod", sig, scale) do c, d_in, d_out
        ccall((:tsdr_invert_am_iq_d, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Cfloat, Csize_t, Ptr{Cvoid}), c.h, d_in, code, scale, n, d_out)
    end
end

"""
    hip_welch_d(d_iq, fmt, scale, nEch, fe; sizeFFT = 1024)
    hip_waterfall_d(d_iq, fmt, scale, nEch, fe; sizeFFT = 1024)

getWelch / getWaterfall of a buffer that already is on the device -- the slot `take_d!` of a raw `HipRing` (`fmt = :sc16raw`,
`:sc8raw`, `:uc8raw`) handed out, the one `hip_frames_submit_iq!` rasters: `fmt` is `:sc16`, `:sc8`, `:uc8` (or `:cf32`), `scale`
the ring's.  The slot is read as stored; only the result crosses PCIe.
"""
function hip_welch_d(d_iq::Ptr{Cvoid}, fmt::Symbol, scale::Real, nEch::Integer, fe; sizeFFT = 1024)
    haskey(IQ_FORMATS, fmt) || throw(ArgumentError("unknown IQ format $fmt (:cf32, :sc16, :sc8, :uc8)"))
    c = ctx(); y = Vector{Float32}(undef, sizeFFT)
    d_y = ccall((:tsdr_dev_alloc, LIB), Ptr{Cvoid}, (Ptr{Cvoid}, Csize_t), c.h, sizeof(y))
    d_y == C_NULL && throw(OutOfMemoryError())
    try
        check(c, ccall((:tsdr_welch_iq_d, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Cfloat, Csize_t, Csize_t, Cint, Ptr{Cvoid}),
                       c.h, d_iq, IQ_FORMATS[fmt], Float32(scale), nEch, sizeFFT, 0, d_y), "getWelch")
        check(c, ccall((:tsdr_download, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Csize_t), c.h, y, d_y, sizeof(y)), "download")
    finally
        ccall((:tsdr_dev_free, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}), c.h, d_y)
    end
    return (collect(((0:sizeFFT-1) ./ sizeFFT .- 0.5) * fe), y)
end
function hip_waterfall_d(d_iq::Ptr{Cvoid}, fmt::Symbol, scale::Real, nEch::Integer, fe; sizeFFT = 1024)
    haskey(IQ_FORMATS, fmt) || throw(ArgumentError("unknown IQ format $fmt (:cf32, :sc16, :sc8, :uc8)"))
    nbSeg = nEch ÷ sizeFFT
    c = ctx(); m = Matrix{Float64}(undef, sizeFFT, nbSeg)
    d_m = ccall((:tsdr_dev_alloc, LIB), Ptr{Cvoid}, (Ptr{Cvoid}, Csize_t), c.h, max(sizeof(m), 8))
    d_m == C_NULL && throw(OutOfMemoryError())
    try
        check(c, ccall((:tsdr_waterfall_iq_d, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Cfloat, Csize_t, Csize_t, Ptr{Cvoid}),
                       c.h, d_iq, IQ_FORMATS[fmt], Float32(scale), nEch, sizeFFT, d_m), "getWaterfall")
        check(c, ccall((:tsdr_download, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Csize_t), c.h, m, d_m, sizeof(m)), "download")
    finally
        ccall((:tsdr_dev_free, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}), c.h, d_m)
    end
    return ((0:nbSeg-1) * (sizeFFT / fe), collect(((0:sizeFFT-1) ./ sizeFFT .- 0.5) .* fe), m)
end
