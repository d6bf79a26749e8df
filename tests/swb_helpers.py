"""Helpers of the dgen_size_with_batt tests: scipy's bounded scalar minimiser
restated in plain Python floats, so that a search can be replayed over a table
of recorded (x, f) pairs and its requests compared one by one."""
import math


def _sign(v):
    return 1.0 if v > 0.0 else (-1.0 if v < 0.0 else 0.0)


def bounded_brent(f, lo, hi, xatol, maxfun=500):
    """scipy.optimize._optimize._minimize_scalar_bounded (1.15), operation for
    operation on Python floats: minimise f over [lo, hi].  Returns (xs, xf,
    nfev): the requested x's in order, the minimiser (always one of xs) and
    the number of evaluations."""
    sqrt_eps = math.sqrt(2.2e-16)
    golden_mean = 0.5 * (3.0 - math.sqrt(5.0))
    a, b = float(lo), float(hi)
    fulc = a + golden_mean * (b - a)
    nfc, xf = fulc, fulc
    rat = e = 0.0
    x = xf
    xs = [x]
    fx = f(x)
    num = 1
    ffulc = fnfc = fx
    xm = 0.5 * (a + b)
    tol1 = sqrt_eps * abs(xf) + xatol / 3.0
    tol2 = 2.0 * tol1
    while abs(xf - xm) > (tol2 - 0.5 * (b - a)):
        golden = True
        if abs(e) > tol1:
            golden = False
            r = (xf - nfc) * (fx - ffulc)
            q = (xf - fulc) * (fx - fnfc)
            p = (xf - fulc) * q - (xf - nfc) * r
            q = 2.0 * (q - r)
            if q > 0.0:
                p = -p
            q = abs(q)
            r = e
            e = rat
            if (abs(p) < abs(0.5 * q * r)) and (p > q * (a - xf)) and (p < q * (b - xf)):
                rat = (p + 0.0) / q
                x = xf + rat
                if ((x - a) < tol2) or ((b - x) < tol2):
                    si = _sign(xm - xf) + (1.0 if (xm - xf) == 0.0 else 0.0)
                    rat = tol1 * si
            else:
                golden = True
        if golden:
            e = (a - xf) if xf >= xm else (b - xf)
            rat = golden_mean * e
        si = _sign(rat) + (1.0 if rat == 0.0 else 0.0)
        x = xf + si * max(abs(rat), tol1)
        xs.append(x)
        fu = f(x)
        num += 1
        if fu <= fx:
            if x >= xf:
                a = xf
            else:
                b = xf
            fulc, ffulc = nfc, fnfc
            nfc, fnfc = xf, fx
            xf, fx = x, fu
        else:
            if x < xf:
                a = x
            else:
                b = x
            if (fu <= fnfc) or (nfc == xf):
                fulc, ffulc = nfc, fnfc
                nfc, fnfc = x, fu
            elif (fu <= ffulc) or (fulc == xf) or (fulc == nfc):
                fulc, ffulc = x, fu
        xm = 0.5 * (a + b)
        tol1 = sqrt_eps * abs(xf) + xatol / 3.0
        tol2 = 2.0 * tol1
        if num >= maxfun:
            break
    return xs, xf, num


def xatol_of(lo, hi):
    """The sizing call's tolerance (financial_functions.py:444) on Python floats."""
    return max(2.0, float(math.floor(max(1.0, hi - lo) * 1e-3)))
