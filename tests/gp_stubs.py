"""Stand-ins shared by the CPU tests of the posterior consumers: a device context that is only a lock, and the
squared-exponential GP those tests build."""

import threading


class _NoDevice:
    """Stands in for the device context: the refusals below must come before any device work."""

    lock = threading.RLock()


def _se_gp(D=2, iso=False, quirks=False, mean=None):
    import gpyreg_amd as gpr

    cov = gpr.isotropic_covariance_functions.SquaredExponentialIsotropic() if iso else \
        gpr.covariance_functions.SquaredExponential()
    return gpr.GP(D, cov, mean or gpr.mean_functions.ConstantMean(),
                  gpr.noise_functions.GaussianNoise(constant_add=True), reference_quirks=quirks)
