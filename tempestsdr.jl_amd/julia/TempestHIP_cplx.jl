# TempestHIP_cplx.jl -- part of module TempestHIP (included at its end): the `ccall`s of include/tempest_hip_cplx.h,
# calculate_autocorrelation (Autocorrelations.jl:23-37) of COMPLEX input.  The reference function is untyped, and
# ifft(fft(x) .* conj(fft(x))) is defined for a complex x: the coherent autocorrelation of the IQ samples themselves, which a user
# gets by calling it on sigRx.  Return shape and exceptions are those of the Float32 method in TempestHIP.jl.

function _autocorr_window(Fs, minDelay, maxDelay)
    indexMin = 1 + round(minDelay * Fs) |> Int
    indexMax = round(maxDelay * Fs) |> Int
    return indexMin, indexMax
end

function calculate_autocorrelation(x::AbstractVector{ComplexF32}, Fs, minDelay, maxDelay, scale = :log)
    xv = _dense(x)
    indexMin, indexMax = _autocorr_window(Fs, minDelay, maxDelay)
    out = Vector{Float32}(undef, max(indexMax - indexMin + 1, 1)); n = Ref{Csize_t}(0); c = ctx()
    check(c, ccall((:tsdr_autocorr_cplx, LIB), Cint,
                   (Ptr{Cvoid}, Ptr{ComplexF32}, Csize_t, Cdouble, Cdouble, Cdouble, Cint, Ptr{Float32}, Ptr{Csize_t}),
                   c.h, xv, length(xv), Fs, minDelay, maxDelay, scale == :log ? 1 : 0, out, n), "calculate_autocorrelation")
    lags = (0:(indexMax - indexMin)) * 1 / Fs
    return resize!(out, n[]), lags
end
function calculate_autocorrelation(x::AbstractVector{ComplexF64}, Fs, minDelay, maxDelay, scale = :log)
    xv = _dense(x)
    indexMin, indexMax = _autocorr_window(Fs, minDelay, maxDelay)
    out = Vector{Float64}(undef, max(indexMax - indexMin + 1, 1)); n = Ref{Csize_t}(0); c = ctx()
    check(c, ccall((:tsdr_autocorr_cplx_f64, LIB), Cint,
                   (Ptr{Cvoid}, Ptr{ComplexF64}, Csize_t, Cdouble, Cdouble, Cdouble, Cint, Ptr{Float64}, Ptr{Csize_t}),
                   c.h, xv, length(xv), Fs, minDelay, maxDelay, scale == :log ? 1 : 0, out, n), "calculate_autocorrelation")
    lags = (0:(indexMax - indexMin)) * 1 / Fs
    return resize!(out, n[]), lags
end
# Integer IQ as the SDR stored it: the raw samples go up (2 or 4 bytes each) and every component is (Float32(code) - offset) * scale
# in the transform's loader.  (The keyword is `scale` as in getSpectrum; the positional lin / log switch is `logscale` here.)
function calculate_autocorrelation(x::AbstractVector{<:IntIQ}, Fs, minDelay, maxDelay, logscale = :log; scale::Float32 = 1f0)
    xv = _dense(x)
    indexMin, indexMax = _autocorr_window(Fs, minDelay, maxDelay)
    out = Vector{Float32}(undef, max(indexMax - indexMin + 1, 1)); n = Ref{Csize_t}(0); c = ctx()
    check(c, ccall((:tsdr_autocorr_cplx_iq, LIB), Cint,
                   (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Cfloat, Csize_t, Cdouble, Cdouble, Cdouble, Cint, Ptr{Float32}, Ptr{Csize_t}),
                   c.h, xv, _iq_code(xv), scale, length(xv), Fs, minDelay, maxDelay, logscale == :log ? 1 : 0, out, n), "calculate_autocorrelation")
    lags = (0:(indexMax - indexMin)) * 1 / Fs
    return resize!(out, n[]), lags
end
