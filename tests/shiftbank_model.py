"""A numpy float32 model of one stream of the shifter bank (csdr_amd_shiftbank): shift_addition_cc / _fc (libcsdr_gpl.c:27-79), shift_math_cc
(libcsdr.c:186-207) and shift_table_cc (libcsdr.c:229-265) with the state carried across calls, so that the result does not depend on how calls cut the
stream, and the bank's retune rule.  Every operation is one float32 operation in the reference's order; cos and sin are libm's double functions
(math.cos / math.sin) rounded to float32, as the reference calls them."""
import math
import numpy as np

f32 = np.float32
c64 = np.complex64
PI = f32(3.14159265358979323846)
TWO_PI = f32(2) * PI

RATES = [0.0, 4e-4, -0.085, 0.3141, 0.5, -0.5, 1.7, 1e-7]


def wrap_pm_pi(p):
    p = f32(p)
    while p > PI: p = f32(p - TWO_PI)
    while p < -PI: p = f32(p + TWO_PI)
    return p


def wrap_0_2pi(p):
    p = f32(p)
    while p > TWO_PI: p = f32(p - TWO_PI)
    while p < 0: p = f32(p + TWO_PI)
    return p


def inc_of(rate):
    return f32(f32(f32(rate) * f32(2)) * PI)


def fcos(x): return f32(math.cos(float(x)))
def fsin(x): return f32(math.sin(float(x)))


def advance(phase, rate, length):
    """the phase after `length` samples of a chunk: phase + rate*PI*length, wrapped (libcsdr_gpl.c:48-51)"""
    return wrap_pm_pi(f32(f32(phase) + f32(inc_of(rate) * f32(length))))


def end_phase(variant, st):
    """what the reference would hand back had the stream ended here: ADDITION closes the open chunk (the record's phase is the chunk's start)"""
    if variant == "addition" and st.pos > 0:
        return advance(st.phase, st.old_rate, st.pos)
    return f32(st.phase)


def quarter_table(size):
    return np.array([fsin(f32(f32(f32(k) / f32(size)) * f32(PI / f32(2)))) for k in range(size)], f32)


class ShiftModel:
    def __init__(self, variant, rate, chunk=1024, table_size=65536, real=False, phase=0.0):
        self.variant, self.chunk, self.real = variant, (chunk if variant == "addition" else 1), real
        self.rate = self.old_rate = f32(rate)
        self.phase, self.c, self.s, self.pos, self.pending = f32(phase), f32(1), f32(0), 0, 0
        self.table = quarter_table(table_size) if variant == "table" else None

    def set_rate(self, rate):
        self.rate, self.pending = f32(rate), 1

    def record(self):
        return (f32(self.rate), f32(self.phase), f32(self.c), f32(self.s), self.pos, self.pending, f32(self.old_rate))

    def _rot(self, p):
        if self.variant == "math":
            return fcos(p), fsin(p)
        size, q90 = self.table.size, f32(PI / f32(2))
        quadrant = int(f32(p / q90))
        within = f32(p - f32(f32(quadrant) * q90))
        si = int(f32(f32(within / q90) * f32(size))); ci = size - 1 - si
        if quadrant & 1: si, ci = ci, si
        si = min(max(si, 0), size - 1); ci = min(max(ci, 0), size - 1)
        s = f32((-1.0 if quadrant > 1 else 1.0)) * self.table[si]
        c = f32((-1.0 if quadrant and quadrant < 3 else 1.0)) * self.table[ci]
        return f32(c), f32(s)

    def process(self, x):
        x = np.asarray(x)
        y = np.zeros(x.size, c64)
        if not x.size:
            return y
        xr = x.real.astype(f32); xi = np.zeros(x.size, f32) if self.real else x.imag.astype(f32)
        if self.variant == "addition":
            if self.pending:
                if self.pos > 0: self.phase = advance(self.phase, self.old_rate, self.pos)
                self.pos = self.pending = 0
            self.old_rate = self.rate
            inc = inc_of(self.rate)
            sd, cd = fsin(inc), fcos(inc)
            c, s = self.c, self.s
            for j in range(x.size):
                if self.pos == 0: c, s = fcos(self.phase), fsin(self.phase)
                if self.real: y[j] = complex(f32(c * xr[j]), f32(s * xr[j]))
                else: y[j] = complex(f32(f32(c * xr[j]) - f32(s * xi[j])), f32(f32(s * xr[j]) + f32(c * xi[j])))
                c, s = f32(f32(c * cd) - f32(s * sd)), f32(f32(s * cd) + f32(c * sd))
                self.pos += 1
                if self.pos == self.chunk:
                    self.phase = advance(self.phase, self.rate, self.chunk); self.pos = 0
            self.c, self.s = c, s
        else:
            inc, p = inc_of(self.rate), self.phase
            for j in range(x.size):
                c, s = self._rot(p)
                y[j] = complex(f32(f32(c * xr[j]) - f32(s * xi[j])), f32(f32(s * xr[j]) + f32(c * xi[j])))
                p = wrap_0_2pi(f32(p + inc))
            self.phase, self.c, self.s, self.pos, self.pending, self.old_rate = p, f32(1), f32(0), 0, 0, self.rate
        return y
