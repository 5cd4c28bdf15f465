# TempestHIP.jl -- thin `ccall` shim over libtempest_hip.so (include/tempest_hip.h).
#
# Re-exports TempestSDR.jl's hot-path functions with the reference's own names and argument
# lists, so that GUI.jl / production scripts run unmodified once TempestSDR.jl does
#
#     include("TempestHIP.jl"); using .TempestHIP          # instead of include("Demodulation.jl") etc.
#
# (see INTEGRATION.md).  Julia is not available in the build container, so this file has not
# been executed there; its Python twin tempestsdr.jl_amd/api.py binds the same entry points with
# the same conventions and IS exercised by the test-suite.  Keep the two in step.
# julia/runtests.jl replays tests/golden/v2 through this shim on a machine that has Julia and a GPU.
#
# Conventions (tempest_hip.h): status 0 = ok; -1 -> AssertionError/ArgumentError, -2 -> BoundsError;
# ComplexF32 vectors are passed as-is (interleaved f32); matrices are column-major, as here.
module TempestHIP

export amDemod, invert_amDemod, fmDemod
export sig_to_image, downgradeImage, naiveResampler, init_resampler
export calculate_autocorrelation, zoom_autocorr
export getSpectrum, getWelch, getWaterfall
export hip_welch_d, hip_waterfall_d                                   # getWelch / getWaterfall of a device buffer in any IQ format (a raw ring slot)
export SyncXY, vsync
export hip_frames!, hip_frames_submit!, hip_frames_submit_sc16!, hip_frames_submit_iq!, hip_frames_flush, hip_synchronize   # fused GUI.jl:163-178 loop body (optional fast path; pipelined form)
export hip_extract_configuration, sync_guard_stats, sync_guard_auto, wait_stats, frames_overlap_stats, debug_hold_tail  # fused GUI.jl:67-81 search; counters of the FAST loop's sync guard
export hip_set_precision, hip_set_option                              # TSDR_EXACT / TSDR_FAST and the library's options, per task context
export arg_area_blank!                                                # FrameSynchronisation.jl:53's binding: findmax (bright blanking) or findmin
export HipGroup, hip_group                                            # one process, several GPUs (RCCL inside the library): `devices = ...`
export hip_abs2, hip_imresize, hip_sync_beta, hip_fill_beta                 # Float64 / ComplexF64 helpers (abs2, imresize, beta fields, fill_beta!)

const LIB = get(ENV, "TEMPEST_HIP_LIB", joinpath(@__DIR__, "..", "libtempest_hip.so"))
const RENDERING_SIZE = (600, 800)   # GUI.jl:10

# ---- context: one per TASK.  The frame loop runs in a `Threads.@spawn`ed task (GUI.jl:381) and the configuration
# search in an Observable callback on the main task (GUI.jl:411-419); tasks may migrate between OS threads
# (Julia >= 1.7), so the key is the task, not Threads.threadid().  A tsdr_ctx is not re-entrant.
mutable struct Ctx
    h::Ptr{Cvoid}
end
function Ctx(device::Integer = 0)
    h = ccall((:tsdr_create, LIB), Ptr{Cvoid}, (Cint,), device)
    h == C_NULL && error("tempest_hip: no usable HIP device (there is no CPU fallback)")
    c = Ctx(h)
    finalizer(c) do x
        # children (SyncXY, resamplers, rings) test c.h before freeing themselves: finalizers run in no particular order
        if x.h != C_NULL
            ccall((:tsdr_destroy, LIB), Cvoid, (Ptr{Cvoid},), x.h)
            x.h = C_NULL
        end
    end
    return c
end
ctx() = get!(() -> Ctx(parse(Int, get(ENV, "TEMPEST_HIP_DEVICE", "0"))), task_local_storage(), :tempest_hip_ctx)::Ctx

# what the reference would have thrown: -1 -> AssertionError (@assert / MethodError sites), -2 -> BoundsError
function check(c::Ctx, rc::Cint, what)
    rc == 0 && return
    detail = unsafe_string(ccall((:tsdr_last_error, LIB), Cstring, (Ptr{Cvoid},), c.h))
    msg = "$what: " * unsafe_string(ccall((:tsdr_strerror, LIB), Cstring, (Cint,), rc)) * " [$detail]"
    rc == -1 && throw(AssertionError(msg))
    rc == -2 && throw(BoundsError(what, detail))   # BoundsError(a, i): "attempt to access <what> at index [<detail>]"
    rc == -3 && throw(OutOfMemoryError())
    error(msg)
end

# dense storage without a copy when the argument already is one: Arrays, and contiguous views such as the
# `@views sigAbs[(n-1)*S .+ (1:S)]` of GUI.jl:166 (ccall takes their pointer directly)
_dense(a::Array) = a
_dense(a::SubArray{T,1,<:Array,<:Tuple{AbstractUnitRange},true}) where {T} = a
_dense(a::AbstractArray) = collect(a)

# ---- Demodulation.jl --------------------------------------------------------------------
function amDemod(sig::Array{ComplexF32})                      # Demodulation.jl:26-28
    out = similar(sig, Float32); c = ctx()
    check(c, ccall((:tsdr_am_demod, LIB), Cint, (Ptr{Cvoid}, Ptr{ComplexF32}, Csize_t, Ptr{Float32}), c.h, sig, length(sig), out), "amDemod")
    return out
end
function invert_amDemod(sig::Array{ComplexF32})               # Demodulation.jl:31-35
    out = similar(sig, Float32); c = ctx()
    check(c, ccall((:tsdr_invert_am, LIB), Cint, (Ptr{Cvoid}, Ptr{ComplexF32}, Csize_t, Ptr{Float32}), c.h, sig, length(sig), out), "invert_amDemod")
    return out
end
function fmDemod(sig::Array{ComplexF32})                      # Demodulation.jl:17-23
    out = similar(sig, Float32); c = ctx()
    check(c, ccall((:tsdr_fm_demod, LIB), Cint, (Ptr{Cvoid}, Ptr{ComplexF32}, Csize_t, Ptr{Float32}), c.h, sig, length(sig), out), "fmDemod")
    return out
end

# ComplexF64 (a `readComplexBinary(file, :double)` capture, DatBinaryFiles.jl:53-64): the `_f64` entry points, Float64 out
function amDemod(sig::Array{ComplexF64})
    out = similar(sig, Float64); c = ctx()
    check(c, ccall((:tsdr_am_demod_f64, LIB), Cint, (Ptr{Cvoid}, Ptr{ComplexF64}, Csize_t, Ptr{Float64}), c.h, sig, length(sig), out), "amDemod")
    return out
end
function invert_amDemod(sig::Array{ComplexF64})
    out = similar(sig, Float64); c = ctx()
    check(c, ccall((:tsdr_invert_am_f64, LIB), Cint, (Ptr{Cvoid}, Ptr{ComplexF64}, Csize_t, Ptr{Float64}), c.h, sig, length(sig), out), "invert_amDemod")
    return out
end
function fmDemod(sig::Array{ComplexF64})
    out = similar(sig, Float64); c = ctx()
    check(c, ccall((:tsdr_fm_demod_f64, LIB), Cint, (Ptr{Cvoid}, Ptr{ComplexF64}, Csize_t, Ptr{Float64}), c.h, sig, length(sig), out), "fmDemod")
    return out
end
"`abs2.(sig)` on the device (GUI.jl:70); Float64 for ComplexF64 input"
function hip_abs2(sig::Array{ComplexF64})
    out = similar(sig, Float64); c = ctx()
    check(c, ccall((:tsdr_abs2_f64, LIB), Cint, (Ptr{Cvoid}, Ptr{ComplexF64}, Csize_t, Ptr{Float64}), c.h, sig, length(sig), out), "abs2")
    return out
end

# ---- Resampler.jl -----------------------------------------------------------------------
function sig_to_image(sig::AbstractVector{Float32}, y_t, x_t)   # Resampler.jl:117-122
    s = _dense(sig)
    img = Matrix{Float32}(undef, Int(y_t), Int(x_t)); c = ctx()
    check(c, ccall((:tsdr_sig_to_image, LIB), Cint, (Ptr{Cvoid}, Ptr{Float32}, Csize_t, Cint, Cint, Ptr{Float32}),
                   c.h, s, length(s), y_t, x_t, img), "sig_to_image")
    return img
end
function downgradeImage(image::AbstractMatrix{Float32})         # Resampler.jl:124-126
    a = _dense(image); out = Matrix{Float32}(undef, RENDERING_SIZE...); c = ctx()
    check(c, ccall((:tsdr_downgrade, LIB), Cint, (Ptr{Cvoid}, Ptr{Float32}, Cint, Cint, Ptr{Float32}),
                   c.h, a, size(a, 1), size(a, 2), out), "downgradeImage")
    return out
end
function naiveResampler(sigOut::Vector{Float32}, sigId::Vector{Float32}, upCoeff)   # Resampler.jl:103-110
    length(sigOut) >= upCoeff * length(sigId) || throw(BoundsError(sigOut, upCoeff * length(sigId)))
    c = ctx()
    check(c, ccall((:tsdr_naive_resample, LIB), Cint, (Ptr{Cvoid}, Ptr{Float32}, Csize_t, Cint, Ptr{Float32}),
                   c.h, sigId, length(sigId), upCoeff, sigOut), "naiveResampler")
    return nothing
end
# Float64 (imresize keeps the element type it is given)
function sig_to_image(sig::AbstractVector{Float64}, y_t, x_t)
    s = _dense(sig)
    img = Matrix{Float64}(undef, Int(y_t), Int(x_t)); c = ctx()
    check(c, ccall((:tsdr_sig_to_image_f64, LIB), Cint, (Ptr{Cvoid}, Ptr{Float64}, Csize_t, Cint, Cint, Ptr{Float64}),
                   c.h, s, length(s), y_t, x_t, img), "sig_to_image")
    return img
end
function downgradeImage(image::AbstractMatrix{Float64})
    a = _dense(image); out = Matrix{Float64}(undef, RENDERING_SIZE...); c = ctx()
    check(c, ccall((:tsdr_downgrade_f64, LIB), Cint, (Ptr{Cvoid}, Ptr{Float64}, Cint, Cint, Ptr{Float64}),
                   c.h, a, size(a, 1), size(a, 2), out), "downgradeImage")
    return out
end
function naiveResampler(sigOut::Vector{Float64}, sigId::Vector{Float64}, upCoeff)
    length(sigOut) >= upCoeff * length(sigId) || throw(BoundsError(sigOut, upCoeff * length(sigId)))
    c = ctx()
    check(c, ccall((:tsdr_naive_resample_f64, LIB), Cint, (Ptr{Cvoid}, Ptr{Float64}, Csize_t, Cint, Ptr{Float64}),
                   c.h, sigId, length(sigId), upCoeff, sigOut), "naiveResampler")
    return nothing
end
"`imresize(sig, n_out)` on a Float64 vector (the 1-D core of sig_to_image, Resampler.jl:119)"
function hip_imresize(sig::AbstractVector{Float64}, n_out::Integer)
    s = _dense(sig); out = Vector{Float64}(undef, n_out); c = ctx()
    check(c, ccall((:tsdr_resize1d_f64, LIB), Cint, (Ptr{Cvoid}, Ptr{Float64}, Csize_t, Csize_t, Ptr{Float64}),
                   c.h, s, length(s), n_out, out), "imresize")
    return out
end
"`imresize(image, (h_out, w_out))` on a Float64 matrix (Resampler.jl:125)"
function hip_imresize(image::AbstractMatrix{Float64}, sz::Tuple{Integer,Integer})
    a = _dense(image); out = Matrix{Float64}(undef, sz[1], sz[2]); c = ctx()
    check(c, ccall((:tsdr_resize2d_f64, LIB), Cint, (Ptr{Cvoid}, Ptr{Float64}, Cint, Cint, Cint, Cint, Ptr{Float64}),
                   c.h, a, size(a, 1), size(a, 2), sz[1], sz[2], out), "imresize")
    return out
end
function init_resampler(T::Type, bufferSize::Int, upCoeff::Int)  # Resampler.jl:26-62
    T == Float32 || T == Float64 || throw(AssertionError("the HIP path implements Float32 and Float64 resamplers"))
    T == Float64 && return _init_resampler64(bufferSize, upCoeff)
    c = ctx(); r = Ref{Ptr{Cvoid}}(C_NULL)
    check(c, ccall((:tsdr_resampler_init, LIB), Cint, (Ptr{Cvoid}, Csize_t, Cint, Ptr{Ptr{Cvoid}}), c.h, bufferSize, upCoeff, r), "init_resampler")
    h = r[]
    keep = Ref(c)                           # the closure keeps its context alive
    finalizer(keep) do k                    # and the native state goes with the closure
        k[].h != C_NULL && ccall((:tsdr_resampler_free, LIB), Cvoid, (Ptr{Cvoid},), h)
    end
    function resampler!(out::AbstractVector{T2}, in::AbstractVector{T2}) where T2
        keep[] === c || error("unreachable")
        @assert T == T2 "Type of input ($T2) should match type used during init ($T)"             # :44
        @assert length(in) == bufferSize "Size of input $(length(in)) should match size used during init $bufferSize"   # :47
        check(c, ccall((:tsdr_resampler_run, LIB), Cint, (Ptr{Cvoid}, Ptr{Float32}, Csize_t, Ptr{Float32}), h, in, length(in), out), "resampler!")
    end
    return resampler!
end
# init_resampler(Float64, ...): the same H; containerFFT in ComplexF64 (tsdr_resampler_init_f64 / tsdr_resampler_run_f64)
function _init_resampler64(bufferSize::Int, upCoeff::Int)
    T = Float64
    c = ctx(); r = Ref{Ptr{Cvoid}}(C_NULL)
    check(c, ccall((:tsdr_resampler_init_f64, LIB), Cint, (Ptr{Cvoid}, Csize_t, Cint, Ptr{Ptr{Cvoid}}), c.h, bufferSize, upCoeff, r), "init_resampler")
    h = r[]
    keep = Ref(c)
    finalizer(keep) do k
        k[].h != C_NULL && ccall((:tsdr_resampler_free, LIB), Cvoid, (Ptr{Cvoid},), h)
    end
    function resampler!(out::AbstractVector{T2}, in::AbstractVector{T2}) where T2
        keep[] === c || error("unreachable")
        @assert T == T2 "Type of input ($T2) should match type used during init ($T)"             # :44
        @assert length(in) == bufferSize "Size of input $(length(in)) should match size used during init $bufferSize"   # :47
        check(c, ccall((:tsdr_resampler_run_f64, LIB), Cint, (Ptr{Cvoid}, Ptr{Float64}, Csize_t, Ptr{Float64}), h, in, length(in), out), "resampler!")
    end
    return resampler!
end
init_resampler(x::Vector{T}, upCoeff) where T = init_resampler(T, length(x), upCoeff)   # :65-68

# ---- Autocorrelations.jl ------------------------------------------------------------------
# Element types.  The reference's functions are generic in T; its own callers (GUI.jl, production/) only ever pass
# Float32 / ComplexF32; the offline flow of production/investigate_data.jl also runs on a :double capture, in Float64.  Those
# are the methods this shim defines.  Anything else is a MethodError -- never a silent conversion, which would compute in
# another precision than the reference would have (INTEGRATION.md, section 4).
function calculate_autocorrelation(x::AbstractVector{Float32}, Fs, minDelay, maxDelay, scale = :log)   # Autocorrelations.jl:23-37
    xv = _dense(x)
    indexMin = 1 + round(minDelay * Fs) |> Int
    indexMax = round(maxDelay * Fs) |> Int
    out = Vector{Float32}(undef, max(indexMax - indexMin + 1, 1)); n = Ref{Csize_t}(0); c = ctx()
    check(c, ccall((:tsdr_autocorr, LIB), Cint,
                   (Ptr{Cvoid}, Ptr{Float32}, Csize_t, Cdouble, Cdouble, Cdouble, Cint, Ptr{Float32}, Ptr{Csize_t}),
                   c.h, xv, length(xv), Fs, minDelay, maxDelay, scale == :log ? 1 : 0, out, n), "calculate_autocorrelation")
    lags = (0:(indexMax - indexMin)) * 1 / Fs
    return resize!(out, n[]), lags
end
function calculate_autocorrelation(x::AbstractVector{Float64}, Fs, minDelay, maxDelay, scale = :log)
    xv = _dense(x)
    indexMin = 1 + round(minDelay * Fs) |> Int
    indexMax = round(maxDelay * Fs) |> Int
    out = Vector{Float64}(undef, max(indexMax - indexMin + 1, 1)); n = Ref{Csize_t}(0); c = ctx()
    check(c, ccall((:tsdr_autocorr_f64, LIB), Cint,
                   (Ptr{Cvoid}, Ptr{Float64}, Csize_t, Cdouble, Cdouble, Cdouble, Cint, Ptr{Float64}, Ptr{Csize_t}),
                   c.h, xv, length(xv), Fs, minDelay, maxDelay, scale == :log ? 1 : 0, out, n), "calculate_autocorrelation")
    lags = (0:(indexMax - indexMin)) * 1 / Fs
    return resize!(out, n[]), lags
end
function zoom_autocorr(Γ, Fs; rate_min = 20, rate_max = 100)                 # Autocorrelations.jl:42-53
    pmin = Ref{Csize_t}(0); pmax = Ref{Csize_t}(0)
    rc = ccall((:tsdr_zoom_bounds, LIB), Cint, (Csize_t, Cdouble, Cdouble, Cdouble, Ptr{Csize_t}, Ptr{Csize_t}),
               length(Γ), Fs, rate_min, rate_max, pmin, pmax)
    rc == 0 || throw(BoundsError(Γ, Int(pmin[]):Int(pmax[])))
    xAx = (Int(pmin[]):Int(pmax[])) ./ Fs
    return (1 ./ xAx, Γ[Int(pmin[]):Int(pmax[])])
end

# ---- GetSpectrum.jl -------------------------------------------------------------------------
_raw(sig::AbstractVector{ComplexF32}) = (_dense(sig), 1)
_raw(sig::AbstractVector{Float32}) = (_dense(sig), 0)
_raw(sig::AbstractVector{ComplexF64}) = (_dense(sig), 1)
_raw(sig::AbstractVector{Float64}) = (_dense(sig), 0)
function getSpectrum(fs, sig; N = nothing)                                   # GetSpectrum.jl:21-30
    isnothing(N) && (N = length(sig))
    N <= length(sig) || throw(BoundsError(sig, N))
    a, cplx = _raw(sig); y = Vector{Float32}(undef, N); c = ctx()
    check(c, ccall((:tsdr_spectrum, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Csize_t, Cint, Ptr{Float32}), c.h, a, cplx, N, 0, y), "getSpectrum")
    return (collect(((0:N-1) ./ N .- 0.5) * fs), y)
end
function getSpectrum(fs, sig::AbstractVector{<:Union{Float64,ComplexF64}}; N = nothing)
    isnothing(N) && (N = length(sig))
    N <= length(sig) || throw(BoundsError(sig, N))
    a, cplx = _raw(sig); y = Vector{Float64}(undef, N); c = ctx()
    check(c, ccall((:tsdr_spectrum_f64, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Csize_t, Cint, Ptr{Float64}), c.h, a, cplx, N, 0, y), "getSpectrum")
    return (collect(((0:N-1) ./ N .- 0.5) * fs), y)
end
getSpectrum(sig) = getSpectrum(1, sig)
_raw32(sig::AbstractVector{<:Union{Float32,ComplexF32}}) = _raw(sig)   # the Float32 / ComplexF32 getWelch / getWaterfall; Float64 below
function getWelch(fe, sig; sizeFFT = 1024)                                   # GetSpectrum.jl:36-52
    a, cplx = _raw32(sig); y = Vector{Float32}(undef, sizeFFT); c = ctx()
    check(c, ccall((:tsdr_welch, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Csize_t, Csize_t, Cint, Ptr{Float32}),
                   c.h, a, cplx, length(a), sizeFFT, 0, y), "getWelch")
    return (collect(((0:sizeFFT-1) ./ sizeFFT .- 0.5) * fe), y)
end
function getWaterfall(fe, sig; sizeFFT = 1024)                               # GetSpectrum.jl:54-66
    a, cplx = _raw32(sig); nbSeg = length(a) ÷ sizeFFT
    m = Matrix{Float64}(undef, sizeFFT, nbSeg); c = ctx()
    check(c, ccall((:tsdr_waterfall, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Csize_t, Csize_t, Ptr{Float64}),
                   c.h, a, cplx, length(a), sizeFFT, m), "getWaterfall")
    return ((0:nbSeg-1) * (sizeFFT / fe), collect(((0:sizeFFT-1) ./ sizeFFT .- 0.5) .* fe), m)
end
# Float64 / ComplexF64 (a :double capture): the `_f64` entry points, Float64 out
function getWelch(fe, sig::AbstractVector{<:Union{Float64,ComplexF64}}; sizeFFT = 1024)
    a, cplx = _raw(sig); y = Vector{Float64}(undef, sizeFFT); c = ctx()
    check(c, ccall((:tsdr_welch_f64, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Csize_t, Csize_t, Cint, Ptr{Float64}),
                   c.h, a, cplx, length(a), sizeFFT, 0, y), "getWelch")
    return (collect(((0:sizeFFT-1) ./ sizeFFT .- 0.5) * fe), y)
end
function getWaterfall(fe, sig::AbstractVector{<:Union{Float64,ComplexF64}}; sizeFFT = 1024)
    a, cplx = _raw(sig); nbSeg = length(a) ÷ sizeFFT
    m = Matrix{Float64}(undef, sizeFFT, nbSeg); c = ctx()
    check(c, ccall((:tsdr_waterfall_f64, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Csize_t, Csize_t, Ptr{Float64}),
                   c.h, a, cplx, length(a), sizeFFT, m), "getWaterfall")
    return ((0:nbSeg-1) * (sizeFFT / fe), collect(((0:sizeFFT-1) ./ sizeFFT .- 0.5) .* fe), m)
end
getWaterfall(sig; sizeFFT = 1024) = getWaterfall(1, sig; sizeFFT = sizeFFT)
# Integer IQ as the SDR stored it -- Complex{Int16} (a `:short` capture, DatBinaryFiles.jl:44-66; sc16), Complex{Int8} (sc8),
# Complex{UInt8} (uc8, around 127.5) --: the `_iq` entry points upload the raw 4 or 2 bytes per sample and convert in the
# transform's loader, every component (Float32(code) - offset) * scale.  Float32 out, the axes as above.
const IntIQ = Union{Complex{Int16},Complex{Int8},Complex{UInt8}}
_iq_code(::AbstractVector{Complex{Int16}}) = Cint(1)    # TSDR_IQ_SC16
_iq_code(::AbstractVector{Complex{Int8}}) = Cint(2)     # TSDR_IQ_SC8
_iq_code(::AbstractVector{Complex{UInt8}}) = Cint(3)    # TSDR_IQ_UC8
function getSpectrum(fs, sig::AbstractVector{<:IntIQ}; N = nothing, scale::Float32 = 1f0)
    isnothing(N) && (N = length(sig))
    N <= length(sig) || throw(BoundsError(sig, N))
    a = _dense(sig); y = Vector{Float32}(undef, N); c = ctx()
    check(c, ccall((:tsdr_spectrum_iq, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Cfloat, Csize_t, Cint, Ptr{Float32}),
                   c.h, a, _iq_code(a), scale, N, 0, y), "getSpectrum")
    return (collect(((0:N-1) ./ N .- 0.5) * fs), y)
end
function getWelch(fe, sig::AbstractVector{<:IntIQ}; sizeFFT = 1024, scale::Float32 = 1f0)
    a = _dense(sig); y = Vector{Float32}(undef, sizeFFT); c = ctx()
    check(c, ccall((:tsdr_welch_iq, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Cfloat, Csize_t, Csize_t, Cint, Ptr{Float32}),
                   c.h, a, _iq_code(a), scale, length(a), sizeFFT, 0, y), "getWelch")
    return (collect(((0:sizeFFT-1) ./ sizeFFT .- 0.5) * fe), y)
end
function getWaterfall(fe, sig::AbstractVector{<:IntIQ}; sizeFFT = 1024, scale::Float32 = 1f0)
    a = _dense(sig); nbSeg = length(a) ÷ sizeFFT
    m = Matrix{Float64}(undef, sizeFFT, nbSeg); c = ctx()
    check(c, ccall((:tsdr_waterfall_iq, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Cfloat, Csize_t, Csize_t, Ptr{Float64}),
                   c.h, a, _iq_code(a), scale, length(a), sizeFFT, m), "getWaterfall")
    return ((0:nbSeg-1) * (sizeFFT / fe), collect(((0:sizeFFT-1) ./ sizeFFT .- 0.5) .* fe), m)
end

# ---- FrameSynchronisation.jl ------------------------------------------------------------------
mutable struct SyncXY{T}                                                      # FrameSynchronisation.jl:25-48
    h::Ptr{Cvoid}
    c::Ctx
    y_t::Int
    x_t::Int
    function SyncXY(image::Matrix{T}) where T
        T == Float32 || T == Float64 || throw(MethodError(SyncXY, (image,)))
        c = ctx(); r = Ref{Ptr{Cvoid}}(C_NULL)
        if T == Float64          # SyncXY{Float64}: beta fields in f64 (tsdr_sync_create_f64)
            check(c, ccall((:tsdr_sync_create_f64, LIB), Cint, (Ptr{Cvoid}, Cint, Cint, Ptr{Ptr{Cvoid}}), c.h, size(image, 1), size(image, 2), r), "SyncXY")
        else
            check(c, ccall((:tsdr_sync_create, LIB), Cint, (Ptr{Cvoid}, Cint, Cint, Ptr{Ptr{Cvoid}}), c.h, size(image, 1), size(image, 2), r), "SyncXY")
        end
        s = new{T}(r[], c, size(image, 1), size(image, 2))
        finalizer(s) do x   # tsdr_sync_free touches the context's stream: skip it when the context went first
            x.c.h != C_NULL && ccall((:tsdr_sync_free, LIB), Cvoid, (Ptr{Cvoid},), x.h)
        end
        return s
    end
end
function vsync(image::AbstractMatrix{Float64}, sync::SyncXY{Float64})
    a = _dense(image); sy = Ref{Cint}(0); sx = Ref{Cint}(0)
    size(a) == (sync.y_t, sync.x_t) || throw(DimensionMismatch("image does not match the SyncXY state"))
    check(sync.c, ccall((:tsdr_vsync_f64, LIB), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Cint}, Ptr{Cint}), sync.h, a, sy, sx), "vsync")
    return (Int(sy[]), Int(sx[]))
end
"the beta_x (`:x`) / beta_y (`:y`) field of a SyncXY{Float64}, (w_max - w_min + 1) x n"
function hip_sync_beta(sync::SyncXY{Float64}, which::Symbol)
    # w_min / w_max as SyncXY derives them (FrameSynchronisation.jl:36-41)
    shape = which == :x ? (floor(Int, sync.x_t / 4) - ceil(Int, 5 / 100 * sync.x_t) + 1, sync.x_t) :
                          (floor(Int, sync.y_t / 4) - ceil(Int, 1 / 100 * sync.y_t) + 1, sync.y_t)
    out = Matrix{Float64}(undef, shape...)
    check(sync.c, ccall((:tsdr_sync_beta_f64, LIB), Cint, (Ptr{Cvoid}, Cint, Ptr{Float64}), sync.h, which == :x ? 0 : 1, out), "sync_beta")
    return out
end
"fill_beta!(β, c_v, Sync(w_min, w_max, n)) (FrameSynchronisation.jl:94-112) on Float64 projections -> β"
function hip_fill_beta(cv::AbstractVector{Float64}, n::Integer, w_min::Integer, w_max::Integer)
    x = _dense(cv); β = Matrix{Float64}(undef, w_max - w_min + 1, n); c = ctx()
    check(c, ccall((:tsdr_fill_beta_f64, LIB), Cint, (Ptr{Cvoid}, Ptr{Float64}, Cint, Cint, Cint, Ptr{Float64}), c.h, x, n, w_min, w_max, β), "fill_beta!")
    return β
end
function vsync(image::AbstractMatrix{Float32}, sync::SyncXY{Float32})             # FrameSynchronisation.jl:56-79
    a = _dense(image); sy = Ref{Cint}(0); sx = Ref{Cint}(0)
    size(a) == (sync.y_t, sync.x_t) || throw(DimensionMismatch("image does not match the SyncXY state"))
    check(sync.c, ccall((:tsdr_vsync, LIB), Cint, (Ptr{Cvoid}, Ptr{Float32}, Ptr{Cint}, Ptr{Cint}), sync.h, a, sy, sx), "vsync")
    return (Int(sy[]), Int(sx[]))      # s_y lags one call, exactly as the reference (:66)
end

# ---- fused loop body of coreProcessing (GUI.jl:163-178): optional fast path ----------------------
"""
    hip_frames!(imageOut, sigId, sync, S, y_t, x_t, α; do_align=true) -> (frames, sync_idx)

Replaces GUI.jl:164-178 for one received buffer: `frames[:,:,n]` is what the n-th
`non_blocking_put!(imageOut)` would have carried; `imageOut` is updated in place.
"""
function hip_frames!(imageOut::Matrix{Float32}, sigId::Vector{ComplexF32}, sync::SyncXY{Float32}, S, y_t, x_t, α::Float32; do_align = true)
    nb = length(sigId) ÷ S
    frames = Array{Float32}(undef, RENDERING_SIZE..., nb); idx = Matrix{Cint}(undef, 2, nb); n = Ref{Cint}(0)
    check(sync.c, ccall((:tsdr_frames, LIB), Cint,
                        (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{ComplexF32}, Csize_t, Csize_t, Cint, Cint, Cfloat, Cint, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Cint}, Ptr{Cint}),
                        sync.c.h, sync.h, sigId, length(sigId), S, y_t, x_t, α, do_align ? 1 : 0, imageOut, frames, C_NULL, idx, n), "hip_frames!")
    return frames, idx
end

"""
    hip_frames_submit!(d_imageOut, d_sigId, nEch, sync, S, y_t, x_t, α; d_frames, d_raster = C_NULL, d_idx = C_NULL, do_align = true) -> nb
    hip_frames_flush()

The loop body for callers that stream buffers and keep them on the device (`tsdr_dev_alloc` / `tsdr_upload`): enqueue-only,
pipelined across buffers -- the image launch of this buffer runs beside the vsync statistics / shift + IIR of the previous
one (`tsdr_frames_submit_d`).  Every argument `d_*` is a device pointer; up to three submissions are in flight, each with
its own `d_frames` / `d_raster` / `d_idx`.  Outputs are complete after `hip_frames_flush()` + `hip_synchronize()`.
"""
function hip_frames_submit!(d_imageOut::Ptr{Cvoid}, d_sigId::Ptr{Cvoid}, nEch::Integer, sync::SyncXY{Float32}, S, y_t, x_t, α::Float32;
                            d_frames::Ptr{Cvoid}, d_raster::Ptr{Cvoid} = C_NULL, d_idx::Ptr{Cvoid} = C_NULL, do_align = true)
    n = Ref{Cint}(0)
    check(sync.c, ccall((:tsdr_frames_submit_d, LIB), Cint,
                        (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Csize_t, Csize_t, Cint, Cint, Cfloat, Cint, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cint}),
                        sync.c.h, sync.h, d_sigId, nEch, S, y_t, x_t, α, do_align ? 1 : 0, d_imageOut, d_frames, d_raster, d_idx, n), "hip_frames_submit!")
    return Int(n[])
end
"""
    hip_frames_submit_sc16!(d_imageOut, d_sigId16, scale, nEch, sync, S, y_t, x_t, α; d_frames, ...) -> nb

`hip_frames_submit!` on a device buffer of `nEch` interleaved `Int16` (re, im) pairs -- what SDR hardware delivers, e.g. the
slots of a `HipRing(...; sc16 = true, raw = true)`: every sample is `ComplexF32(re, im) * scale`, formed in the kernels'
loaders, so the buffer is never expanded in HBM (`tsdr_frames_submit_sc16_d`).
"""
function hip_frames_submit_sc16!(d_imageOut::Ptr{Cvoid}, d_sigId16::Ptr{Cvoid}, scale::Float32, nEch::Integer, sync::SyncXY{Float32}, S, y_t, x_t, α::Float32;
                                 d_frames::Ptr{Cvoid}, d_raster::Ptr{Cvoid} = C_NULL, d_idx::Ptr{Cvoid} = C_NULL, do_align = true)
    n = Ref{Cint}(0)
    check(sync.c, ccall((:tsdr_frames_submit_sc16_d, LIB), Cint,
                        (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Cfloat, Csize_t, Csize_t, Cint, Cint, Cfloat, Cint, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cint}),
                        sync.c.h, sync.h, d_sigId16, scale, nEch, S, y_t, x_t, α, do_align ? 1 : 0, d_imageOut, d_frames, d_raster, d_idx, n), "hip_frames_submit_sc16!")
    return Int(n[])
end
"""
    hip_frames_submit_iq!(d_imageOut, d_iq, fmt, scale, nEch, sync, S, y_t, x_t, α; d_frames, ...) -> nb

`hip_frames_submit!` on a device buffer of `nEch` samples of format `fmt` -- `:cf32`, `:sc16` (Int16 pairs), `:sc8` (Int8 pairs:
HackRF, UHD sc8) or `:uc8` (UInt8 pairs around 127.5: RTL-SDR), e.g. the slots of a `HipRing(...; fmt = :sc8raw)`.  Integer
samples become `ComplexF32((I - offset) * scale, (Q - offset) * scale)` in the kernels' loaders (offset 127.5 for `:uc8`, else 0),
so the buffer is never expanded in HBM (`tsdr_frames_submit_iq_d`).
"""
function hip_frames_submit_iq!(d_imageOut::Ptr{Cvoid}, d_iq::Ptr{Cvoid}, fmt::Symbol, scale::Float32, nEch::Integer, sync::SyncXY{Float32}, S, y_t, x_t, α::Float32;
                               d_frames::Ptr{Cvoid}, d_raster::Ptr{Cvoid} = C_NULL, d_idx::Ptr{Cvoid} = C_NULL, do_align = true)
    haskey(IQ_FORMATS, fmt) || throw(ArgumentError("unknown IQ format $fmt (:cf32, :sc16, :sc8, :uc8)"))
    n = Ref{Cint}(0)
    check(sync.c, ccall((:tsdr_frames_submit_iq_d, LIB), Cint,
                        (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Cint, Cfloat, Csize_t, Csize_t, Cint, Cint, Cfloat, Cint, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cint}),
                        sync.c.h, sync.h, d_iq, IQ_FORMATS[fmt], scale, nEch, S, y_t, x_t, α, do_align ? 1 : 0, d_imageOut, d_frames, d_raster, d_idx, n), "hip_frames_submit_iq!")
    return Int(n[])
end
const IQ_FORMATS = Dict(:cf32 => 0, :sc16 => 1, :sc8 => 2, :uc8 => 3)   # TSDR_IQ_*
hip_frames_flush() = (c = ctx(); check(c, ccall((:tsdr_frames_flush, LIB), Cint, (Ptr{Cvoid},), c.h), "hip_frames_flush"))
hip_synchronize() = (c = ctx(); check(c, ccall((:tsdr_synchronize, LIB), Cint, (Ptr{Cvoid},), c.h), "hip_synchronize"))

# ---- fused configuration search (GUI.jl:67-81) ------------------------------------------------------
"""
    hip_extract_configuration(sigId, Fs; delay = 0.1, rate_min = 50, rate_max = 90) -> (rates_refresh, Γ_refresh, fv)

`extract_configuration`'s arithmetic (GUI.jl:67-81) as one library call on the raw IQ: `abs2.` formed while loading,
`calculate_autocorrelation(., Fs, 0, delay)`, `zoom_autocorr(.; rate_min, rate_max)` and `findmax`, the last found by the
launch that writes the lags.
"""
function hip_extract_configuration(sigId::Vector{ComplexF32}, Fs; delay = 0.1, rate_min = 50, rate_max = 90)
    indexMax = round(delay * Fs) |> Int
    Γ = Vector{Float32}(undef, max(indexMax, 1)); n = Ref{Csize_t}(0); c = ctx()
    pmin = Ref{Csize_t}(0); pmax = Ref{Csize_t}(0)
    rc = ccall((:tsdr_zoom_bounds, LIB), Cint, (Csize_t, Cdouble, Cdouble, Cdouble, Ptr{Csize_t}, Ptr{Csize_t}),
               indexMax, Fs, rate_min, rate_max, pmin, pmax)
    rc == 0 || throw(BoundsError(Γ, Int(pmin[]):Int(pmax[])))
    d_in = ccall((:tsdr_dev_alloc, LIB), Ptr{Cvoid}, (Ptr{Cvoid}, Csize_t), c.h, sizeof(sigId))
    d_out = ccall((:tsdr_dev_alloc, LIB), Ptr{Cvoid}, (Ptr{Cvoid}, Csize_t), c.h, sizeof(Γ))
    (d_in == C_NULL || d_out == C_NULL) && throw(OutOfMemoryError())
    idx = Ref{Csize_t}(0); val = Ref{Cfloat}(0)
    try
        check(c, ccall((:tsdr_upload, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Csize_t), c.h, d_in, sigId, sizeof(sigId)), "upload")
        check(c, ccall((:tsdr_autocorr_search_d, LIB), Cint,
                       (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Csize_t, Cdouble, Cdouble, Cdouble, Cint, Ptr{Cvoid}, Ptr{Csize_t}, Csize_t, Csize_t, Ptr{Csize_t}, Ptr{Cfloat}),
                       c.h, d_in, 1, length(sigId), Fs, 0.0, delay, 1, d_out, n, pmin[] - 1, pmax[] - pmin[] + 1, idx, val), "extract_configuration")
        check(c, ccall((:tsdr_download, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Csize_t), c.h, Γ, d_out, n[] * sizeof(Float32)), "download")
    finally
        ccall((:tsdr_dev_free, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}), c.h, d_in)
        ccall((:tsdr_dev_free, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}), c.h, d_out)
    end
    xAx = (Int(pmin[]):Int(pmax[])) ./ Fs
    rates_refresh = 1 ./ xAx
    Γ_refresh = Γ[Int(pmin[]):Int(pmax[])]
    fv = 1 / (1 / rates_refresh[Int(idx[]) + 1])                            # GUI.jl:80-81
    return rates_refresh, Γ_refresh, fv
end
"""
    hip_extract_configuration(d_iq::Ptr{Cvoid}, fmt::Symbol, scale, nEch, Fs; delay = 0.1, rate_min = 50, rate_max = 90)

The same on a raw device buffer of `nEch` samples of format `fmt` (`:sc16`, `:sc8`, `:uc8`; 16-byte aligned, as `take_d!` of a
raw `HipRing` hands out): the first pass of the search converts the stored integers itself, so the search and the frame loop
read one ring and nothing is expanded (`tsdr_autocorr_search_iq_d`).
"""
function hip_extract_configuration(d_iq::Ptr{Cvoid}, fmt::Symbol, scale::Real, nEch::Integer, Fs; delay = 0.1, rate_min = 50, rate_max = 90)
    haskey(IQ_FORMATS, fmt) || throw(ArgumentError("unknown IQ format $fmt (:cf32, :sc16, :sc8, :uc8)"))
    indexMax = round(delay * Fs) |> Int
    Γ = Vector{Float32}(undef, max(indexMax, 1)); n = Ref{Csize_t}(0); c = ctx()
    pmin = Ref{Csize_t}(0); pmax = Ref{Csize_t}(0)
    rc = ccall((:tsdr_zoom_bounds, LIB), Cint, (Csize_t, Cdouble, Cdouble, Cdouble, Ptr{Csize_t}, Ptr{Csize_t}),
               indexMax, Fs, rate_min, rate_max, pmin, pmax)
    rc == 0 || throw(BoundsError(Γ, Int(pmin[]):Int(pmax[])))
    d_out = ccall((:tsdr_dev_alloc, LIB), Ptr{Cvoid}, (Ptr{Cvoid}, Csize_t), c.h, sizeof(Γ))
    d_out == C_NULL && throw(OutOfMemoryError())
    idx = Ref{Csize_t}(0); val = Ref{Cfloat}(0)
    try
        check(c, ccall((:tsdr_autocorr_search_iq_d, LIB), Cint,
                       (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Cfloat, Csize_t, Cdouble, Cdouble, Cdouble, Cint, Ptr{Cvoid}, Ptr{Csize_t}, Csize_t, Csize_t, Ptr{Csize_t}, Ptr{Cfloat}),
                       c.h, d_iq, IQ_FORMATS[fmt], Float32(scale), nEch, Fs, 0.0, delay, 1, d_out, n, pmin[] - 1, pmax[] - pmin[] + 1, idx, val), "extract_configuration")
        check(c, ccall((:tsdr_download, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Csize_t), c.h, Γ, d_out, n[] * sizeof(Float32)), "download")
    finally
        ccall((:tsdr_dev_free, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}), c.h, d_out)
    end
    xAx = (Int(pmin[]):Int(pmax[])) ./ Fs
    rates_refresh = 1 ./ xAx
    Γ_refresh = Γ[Int(pmin[]):Int(pmax[])]
    fv = 1 / (1 / rates_refresh[Int(idx[]) + 1])                            # GUI.jl:80-81
    return rates_refresh, Γ_refresh, fv
end

"""
    hip_set_precision(mode::Symbol)      # :exact (bit-identical to the CPU restatement) or :fast (default; DESIGN.md section 2)

Arithmetic of the frame loop (`hip_frames!`) on this task's context; the per-function entry points always run the exact sequence.
"""
function hip_set_precision(mode::Symbol)
    mode in (:exact, :fast) || throw(ArgumentError("mode must be :exact or :fast"))
    c = ctx()
    check(c, ccall((:tsdr_set_precision, LIB), Cint, (Ptr{Cvoid}, Cint), c.h, mode === :exact ? 0 : 1), "set_precision")
    return mode
end

"`tsdr_set_option` on this task's context: \"sync_guard_ppb\", \"sync_guard_auto\", \"vsync_current_sy\", \"vsync_blank_dark\", \"ac_mixed\", ... (include/tempest_hip.h)"
function hip_set_option(name::AbstractString, value::Integer)
    c = ctx()
    check(c, ccall((:tsdr_set_option, LIB), Cint, (Ptr{Cvoid}, Cstring, Cint), c.h, name, value), "set_option($name)")
    return nothing
end

"""
    arg_area_blank!(findmax)     # the blanking interval is the brightest band (default; the reference as it stands)
    arg_area_blank!(findmin)     # it is the darkest band

The reference's one-word binding `arg_area_blank = findmax` (FrameSynchronisation.jl:51-53) as a setting of this task's
context: option "vsync_blank_dark" of `tsdr_set_option`.  Applies to `vsync` and the frame loop from the next call on; buffers
already submitted keep theirs.  The pending s_y is kept as an index: the first s_y after a change is the old polarity's
(reset the SyncXY for reference-equal behaviour).
"""
function arg_area_blank!(f::Function)
    f === findmin || f === findmax || throw(ArgumentError("arg_area_blank! takes findmin or findmax"))
    hip_set_option("vsync_blank_dark", f === findmin ? 1 : 0)
    return f
end

"(frames checked, frames re-evaluated in the exact sequence) by the TSDR_FAST frame loop's sync guard on this task's context"
function sync_guard_stats(; reset = false)
    a = Ref{Culonglong}(0); b = Ref{Culonglong}(0); c = ctx()
    check(c, ccall((:tsdr_sync_guard_stats, LIB), Cint, (Ptr{Cvoid}, Ptr{Culonglong}, Ptr{Culonglong}, Cint), c.h, a, b, reset ? 1 : 0), "sync_guard_stats")
    return (Int(a[]), Int(b[]))
end

"(whole buffers currently run in the exact sequence?, calls that did, route changes): the sync guard's adaptive route"
function sync_guard_auto()
    e = Ref{Cint}(0); a = Ref{Culonglong}(0); b = Ref{Culonglong}(0); c = ctx()
    check(c, ccall((:tsdr_sync_guard_auto, LIB), Cint, (Ptr{Cvoid}, Ptr{Cint}, Ptr{Culonglong}, Ptr{Culonglong}), c.h, e, a, b), "sync_guard_auto")
    return (e[] != 0, Int(a[]), Int(b[]))
end

"(stream waits given up after \"wait_ms\", guard ring entries that went uncounted): every host-side wait of the library is bounded"
function wait_stats()
    a = Ref{Culonglong}(0); b = Ref{Culonglong}(0); c = ctx()
    check(c, ccall((:tsdr_wait_stats, LIB), Cint, (Ptr{Cvoid}, Ptr{Culonglong}, Ptr{Culonglong}), c.h, a, b), "wait_stats")
    return (Int(a[]), Int(b[]))
end

"(calls on the internal streams, calls on the context's stream, why the latest of those was sequential: bits 1 option or another context on the device, 2 profiling, 4 TSDR_EXACT, 8 adopted stream) of `hip_frames!` on device buffers: option \"frames_overlap\""
function frames_overlap_stats(; reset = false)
    a = Ref{Culonglong}(0); b = Ref{Culonglong}(0); w = Ref{Cuint}(0); c = ctx()
    check(c, ccall((:tsdr_frames_overlap_stats, LIB), Cint, (Ptr{Cvoid}, Ptr{Culonglong}, Ptr{Culonglong}, Ptr{Cuint}, Cint), c.h, a, b, w, reset ? 1 : 0), "frames_overlap_stats")
    return (Int(a[]), Int(b[]), Int(w[]))
end

"diagnostic: the tail of the next frame-loop call on the internal streams starts `ms` milliseconds late (0 disarms)"
function debug_hold_tail(ms::Integer)
    c = ctx()
    check(c, ccall((:tsdr_debug_hold_tail, LIB), Cint, (Ptr{Cvoid}, Cint), c.h, ms), "debug_hold_tail")
    return nothing
end

# ---- one process, several GPUs (tsdr_group_*: one context + one RCCL communicator per device) ----------------------
"""
    HipGroup(devices = 0:0)

What this process holds to use several MI355X of the node (the reference runtime is ONE process, GUI.jl:380-382): one
library context and one RCCL communicator per device (`ncclCommInitAll` inside `libtempest_hip.so`), member 1 (device
`first(devices)`) the root.  Pass it as `group = g` -- or just `devices = 0:7`, which keeps one group per task -- to
`hip_extract_configuration`, `hip_frames!` and `getWelch`:

* the search shards the sum over m of the circular autocorrelation (`Autocorrelations.jl:27-29`), ONE all-reduce of the
  `indexMax` accumulators over xGMI, `10log10(abs2)` and `findmax` after it on the root;
* the frame loop shards the buffer's frames, gathers 600x800 images + argmax keys to the root, which applies the lagged
  `s_y`, `circshift` and the IIR in order.  The group owns its `SyncXY` states (`reset!(g)` = a fresh `SyncXY`).
"""
mutable struct HipGroup
    h::Ptr{Cvoid}
    devices::Vector{Cint}
end
function HipGroup(devices = 0:0)
    devs = collect(Cint, devices); h = Ref{Ptr{Cvoid}}(C_NULL)
    rc = ccall((:tsdr_group_create, LIB), Cint, (Ptr{Cint}, Cint, Ptr{Ptr{Cvoid}}), devs, length(devs), h)
    (rc != 0 || h[] == C_NULL) && error("tempest_hip: tsdr_group_create($(devs)) failed (" *
                                        unsafe_string(ccall((:tsdr_strerror, LIB), Cstring, (Cint,), rc)) * "); there is no CPU fallback")
    g = HipGroup(h[], devs)
    finalizer(g) do x
        if x.h != C_NULL
            ccall((:tsdr_group_destroy, LIB), Cvoid, (Ptr{Cvoid},), x.h)
            x.h = C_NULL
        end
    end
    return g
end
hip_group(devices) = get!(() -> HipGroup(devices), task_local_storage(), (:tempest_hip_group, Tuple(devices)))::HipGroup
Base.length(g::HipGroup) = Int(ccall((:tsdr_group_size, LIB), Cint, (Ptr{Cvoid},), g.h))
function check(g::HipGroup, rc::Cint, what)
    rc == 0 && return
    detail = unsafe_string(ccall((:tsdr_group_last_error, LIB), Cstring, (Ptr{Cvoid},), g.h))
    msg = "$what: " * unsafe_string(ccall((:tsdr_strerror, LIB), Cstring, (Cint,), rc)) * " [$detail]"
    rc == -1 && throw(AssertionError(msg))
    rc == -2 && throw(BoundsError(what, detail))
    rc == -3 && throw(OutOfMemoryError())
    error(msg)
end
reset!(g::HipGroup) = check(g, ccall((:tsdr_group_sync_reset, LIB), Cint, (Ptr{Cvoid},), g.h), "reset!")
hip_set_precision(g::HipGroup, mode::Symbol) =
    check(g, ccall((:tsdr_group_set_precision, LIB), Cint, (Ptr{Cvoid}, Cint), g.h, mode === :exact ? 0 : 1), "set_precision")
hip_set_option(g::HipGroup, name::AbstractString, value::Integer) =
    check(g, ccall((:tsdr_group_set_option, LIB), Cint, (Ptr{Cvoid}, Cstring, Cint), g.h, name, value), "set_option($name)")
"route (:sharded / :root) and the three stage times in ms (per-member stage incl. upload, collective, root's final stage) of the last call"
function timing(g::HipGroup)
    r = Ref{Cint}(0); ms = Vector{Cdouble}(undef, 3)
    check(g, ccall((:tsdr_group_timing, LIB), Cint, (Ptr{Cvoid}, Ptr{Cint}, Ptr{Cdouble}), g.h, r, ms), "timing")
    return (r[] == 1 ? :sharded : :root, ms)
end

"""
    hip_extract_configuration(sigId, Fs; devices, route = :auto, delay = 0.1, rate_min = 50, rate_max = 90)
    hip_extract_configuration(sigId, Fs; group = g, ...)

`extract_configuration`'s arithmetic (GUI.jl:67-81) over several GPUs of this process.  `route = :auto` shards only when a
member's segment + halo transform is smaller than the single-device one (with the reference's own window `n = 2 indexMax`,
`Autocorrelations.jl:27`, it never is -- the root then runs alone); `:sharded` forces the all-reduce route.
"""
function hip_extract_configuration(sigId::Vector{ComplexF32}, Fs, g::HipGroup; route::Symbol = :auto, delay = 0.1, rate_min = 50, rate_max = 90)
    indexMax = round(delay * Fs) |> Int
    Γ = Vector{Float32}(undef, max(indexMax, 1)); n = Ref{Csize_t}(0)
    pmin = Ref{Csize_t}(0); pmax = Ref{Csize_t}(0)
    rc = ccall((:tsdr_zoom_bounds, LIB), Cint, (Csize_t, Cdouble, Cdouble, Cdouble, Ptr{Csize_t}, Ptr{Csize_t}),
               indexMax, Fs, rate_min, rate_max, pmin, pmax)
    rc == 0 || throw(BoundsError(Γ, Int(pmin[]):Int(pmax[])))
    idx = Ref{Csize_t}(0); val = Ref{Cfloat}(0)
    check(g, ccall((:tsdr_group_search, LIB), Cint,
                   (Ptr{Cvoid}, Ptr{ComplexF32}, Cint, Csize_t, Cdouble, Cdouble, Cdouble, Cint, Ptr{Float32}, Ptr{Csize_t}, Csize_t, Csize_t, Ptr{Csize_t}, Ptr{Cfloat}, Cint),
                   g.h, sigId, 1, length(sigId), Fs, 0.0, delay, 1, Γ, n, pmin[] - 1, pmax[] - pmin[] + 1, idx, val,
                   route === :sharded ? 1 : route === :root ? 2 : 0), "extract_configuration")
    xAx = (Int(pmin[]):Int(pmax[])) ./ Fs
    rates_refresh = 1 ./ xAx
    Γ_refresh = Γ[Int(pmin[]):Int(pmax[])]
    fv = 1 / (1 / rates_refresh[Int(idx[]) + 1])                            # GUI.jl:80-81
    return rates_refresh, Γ_refresh, fv
end
hip_extract_configuration(sigId::Vector{ComplexF32}, Fs, devices::AbstractVector{<:Integer}; kw...) =
    hip_extract_configuration(sigId, Fs, hip_group(devices); kw...)

"""
    hip_frames!(imageOut, sigId, g::HipGroup, S, y_t, x_t, α; do_align = true) -> (frames, sync_idx)

`hip_frames!` (GUI.jl:164-178 for one received buffer) with the buffer's frames sharded over the group's devices.
"""
function hip_frames!(imageOut::Matrix{Float32}, sigId::Vector{ComplexF32}, g::HipGroup, S, y_t, x_t, α::Float32; do_align = true)
    nb = length(sigId) ÷ S
    frames = Array{Float32}(undef, RENDERING_SIZE..., nb); idx = Matrix{Cint}(undef, 2, nb); n = Ref{Cint}(0)
    check(g, ccall((:tsdr_group_frames, LIB), Cint,
                   (Ptr{Cvoid}, Ptr{ComplexF32}, Csize_t, Csize_t, Cint, Cint, Cfloat, Cint, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Cint}, Ptr{Cint}),
                   g.h, sigId, length(sigId), S, y_t, x_t, α, do_align ? 1 : 0, imageOut, frames, C_NULL, idx, n), "hip_frames!")
    return frames, idx
end

"getWelch (GetSpectrum.jl:36-52) with the segments sharded over the group: one all-reduce of `sizeFFT` Float32"
function getWelch(fe, sig, g::HipGroup; sizeFFT = 1024)
    a, cplx = _raw(sig)          # (Float32 / ComplexF32 only, like the single-context method: MethodError otherwise)
    y = Vector{Float32}(undef, sizeFFT)
    check(g, ccall((:tsdr_group_welch, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Csize_t, Csize_t, Cint, Ptr{Float32}),
                   g.h, a, cplx, length(a), sizeFFT, 0, y), "getWelch")
    return (collect(((0:sizeFFT-1) ./ sizeFFT .- 0.5) * fe), y)
end

# ---- streaming ingest: the staging ring (AtomicAbstractSDRs.jl:64-190 on pinned memory) ----------
"""
    HipRing(c::Ctx, nEch; depth=16, sc16=false, raw=false, fmt=nothing, scale=1f0)

Pinned-host staging ring with the put/take/overflow semantics of `AtomicCircularBuffer`.  The producer task fills
`write_slot(ring)` in place (e.g. `recv!(write_slot(ring), sdr)`) and calls `commit!(ring)`; the consumer calls
`take_d!(ring)` in place of `recv!(buffer, csdr)` and gets a device pointer to hand to `tsdr_frames_d`.
`fmt = :sc8 | :sc8raw | :uc8 | :uc8raw` (beside `sc16` / `raw`): 8-bit slots, `Int8` pairs or `UInt8` pairs around 127.5, two
bytes per sample -- expanded on the device to `ComplexF32`, or (`raw`) handed out as stored for `hip_frames_submit_iq!` and
`hip_extract_configuration(d_iq, fmt, ...)`.  `fmt` also takes `:cf32`, `:sc16`, `:sc16raw`.
"""
mutable struct HipRing
    c::Ctx
    h::Ptr{Cvoid}
    nEch::Int
    sc16::Bool
    fmt::Symbol
end
const RING_FORMATS = Dict(:cf32 => 0, :sc16 => 1, :sc16raw => 2, :sc8 => 3, :sc8raw => 4, :uc8 => 5, :uc8raw => 6)
function HipRing(c::Ctx, nEch::Integer; depth = 16, sc16 = false, raw = false, fmt::Union{Symbol,Nothing} = nothing, scale = 1f0)
    h = Ref{Ptr{Cvoid}}(C_NULL)   # raw: the integer slots stay as they are on the device (for hip_frames_submit_sc16! / _iq!)
    f = fmt === nothing ? (sc16 ? (raw ? :sc16raw : :sc16) : :cf32) : fmt
    haskey(RING_FORMATS, f) || throw(ArgumentError("unknown ring format $f"))
    check(c, ccall((:tsdr_ring_create, LIB), Cint, (Ptr{Cvoid}, Csize_t, Cint, Cint, Cfloat, Ptr{Ptr{Cvoid}}),
                   c.h, nEch, depth, RING_FORMATS[f], scale, h), "HipRing")
    r = HipRing(c, h[], nEch, f in (:sc16, :sc16raw), f)
    finalizer(r) do x
        x.c.h != C_NULL && ccall((:tsdr_ring_free, LIB), Cvoid, (Ptr{Cvoid},), x.h)
    end
    return r
end
function write_slot(r::HipRing)
    p = ccall((:tsdr_ring_write_ptr, LIB), Ptr{Cvoid}, (Ptr{Cvoid},), r.h)
    r.fmt in (:sc8, :sc8raw) && return unsafe_wrap(Array, Ptr{Int8}(p), 2 * r.nEch)
    r.fmt in (:uc8, :uc8raw) && return unsafe_wrap(Array, Ptr{UInt8}(p), 2 * r.nEch)
    return r.sc16 ? unsafe_wrap(Array, Ptr{Int16}(p), 2 * r.nEch) : unsafe_wrap(Array, Ptr{ComplexF32}(p), r.nEch)
end
commit!(r::HipRing) = check(r.c, ccall((:tsdr_ring_commit, LIB), Cint, (Ptr{Cvoid},), r.h), "commit!")
circ_put!(r::HipRing, data) = check(r.c, ccall((:tsdr_ring_put, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}), r.h, data), "circ_put!")
function take_d!(r::HipRing; timeout_ms = -1)
    d = Ref{Ptr{Cfloat}}(C_NULL)
    check(r.c, ccall((:tsdr_ring_take_d, LIB), Cint, (Ptr{Cvoid}, Cint, Ptr{Ptr{Cfloat}}), r.h, timeout_ms, d), "take_d!")
    return d[]
end

# Integer IQ through the device-pointer `_iq_d` entry points (include/tempest_hip_iq.h): amDemod / invert_amDemod of
# Complex{Int16} / Complex{Int8} / Complex{UInt8} vectors, hip_welch_d / hip_waterfall_d of a raw ring slot
include("TempestHIP_iq.jl")
# calculate_autocorrelation of ComplexF32 / ComplexF64 / integer IQ vectors (include/tempest_hip_cplx.h)
include("TempestHIP_cplx.jl")
# frame averaging at the monitor's own resolution: hip_raster_accumulate!, hip_frames_hires! (include/tempest_hip_hires.h)
include("TempestHIP_hires.jl")
# registration of those rasters to the raster pixel: hip_raster_register!, hip_hires_refine! (include/tempest_hip_register.h)
include("TempestHIP_register.jl")
# display export of any of those pictures: hip_display_u8!, hip_display_u8_d! (include/tempest_hip_display.h)
include("TempestHIP_display.jl")
# coherent folding at a fractional frame period: hip_fold!, hip_fold_d!, hip_fold_scan, hip_fold_scan_d!, fold_plan (include/tempest_hip_fold.h)
include("TempestHIP_fold.jl")
# phase-coherent folding with carrier de-rotation: hip_cfold!, hip_cfold_d!, hip_cfold_scan, hip_cfold_scan_d!, refine_carrier (include/tempest_hip_cfold.h)
include("TempestHIP_cfold.jl")
# coherent stacking across buffers, a complex fold state and a phase lock: hip_cstack!, hip_cstack_d!, cstack_plan (include/tempest_hip_cstack.h)
include("TempestHIP_cstack.jl")
# carrier tracking, a frame phase probe and stacking along a phase track: hip_ctrack_stack!, hip_ctrack_probe, fit_track, constant_track (include/tempest_hip_ctrack.h)
include("TempestHIP_ctrack.jl")
# the frame Gram matrix, blind carrier phases and the κ periodogram from one pass: hip_ctrack_gram, hip_ctrack_gram_d!, gram_energy, gram_carrier, gram_phases, gram_track, track_slopes, blind_track (include/tempest_hip_gram.h)
include("TempestHIP_gram.jl")
# the tuner, frequency shift + FIR low-pass + decimation of an IQ stream chained across calls: hip_tune!, hip_tune_d!, freq_fix, design_lowpass, tune_plan (include/tempest_hip_tune.h)
include("TempestHIP_tune.jl")

end # module
