"""Numpy restatement, in complex128, of getWelch / getWaterfall (GetSpectrum.jl:36-66) and the resampler! closure
(Resampler.jl:26-62) as the `_f64` entry points compute them: numpy's pocketfft in double stands in for FFTW, abs2 is
re*re + im*im, fftshift moves output j to input (j + ceil(N/2)) mod N.  The GPU results are held to this within the bars
of tests/test_f64_spectra_gpu.py (summation orders differ: the bars are relative to the largest value)."""
import numpy as np


def _abs2(X):
    return X.real * X.real + X.imag * X.imag


def _segments(sig, sizeFFT):
    x = np.asarray(sig)
    nb = x.size // sizeFFT
    return x[: nb * sizeFFT].astype(np.complex128).reshape(nb, sizeFFT), nb


def welch(sig, sizeFFT, lin=False):
    """getWelch: sum over the nbSeg = len / sizeFFT whole segments of abs2(fft(segment)), fftshift, 10log10 (or linear);
    no segment: the zero accumulator (-Inf dB)"""
    if sizeFFT <= 0:
        raise ValueError("sizeFFT must be positive")
    segs, nb = _segments(sig, sizeFFT)
    S = np.zeros(sizeFFT, np.float64)
    if nb:
        S = _abs2(np.fft.fft(segs, axis=1)).sum(axis=0)
    S = np.fft.fftshift(S)
    if lin:
        return S
    with np.errstate(divide="ignore"):
        return 10.0 * np.log10(S)


def waterfall(sig, sizeFFT):
    """getWaterfall: column s of the sizeFFT x nbSeg Float64 matrix is fftshift(abs2(fft(segment s))); the tail is dropped"""
    if sizeFFT <= 0:
        raise ValueError("sizeFFT must be positive")
    segs, nb = _segments(sig, sizeFFT)
    if nb == 0:
        return np.zeros((sizeFFT, 0), np.float64, order="F")
    P = np.fft.fftshift(_abs2(np.fft.fft(segs, axis=1)), axes=1)
    return np.asfortranarray(P.T)


def resampler(x, upCoeff, H):
    """resampler!(out, in) with T = Float64: containerFFT[1:up:end] = in (ComplexF64, zero elsewhere); fft; * H (ComplexF64);
    ifft (1/N); out = 2 upCoeff real(.)"""
    x = np.asarray(x, np.float64)
    N = x.size * int(upCoeff)
    H = np.asarray(H, np.complex128)
    assert H.size == N
    c = np.zeros(N, np.complex128)
    c[:: int(upCoeff)] = x
    return 2 * int(upCoeff) * np.fft.ifft(np.fft.fft(c) * H).real
