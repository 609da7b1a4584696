"""normflow 1.2, distributions/linear_interpolation.py: the geometric bridge between two densities."""


class LinearInterpolation:
    """Linear interpolation of two distributions in the log space: alpha log p1 + (1 - alpha) log p2.

    A plain object, not a module, as in the reference: a layer that holds one (the HamiltonianMonteCarlo layers of
    vcnf_amd.sampling.HAIS) does not register the parameters of ``dist1`` or ``dist2`` as its own."""

    def __init__(self, dist1, dist2, alpha):
        self.alpha = alpha
        self.dist1 = dist1
        self.dist2 = dist2

    def log_prob(self, z):
        return self.alpha * self.dist1.log_prob(z) + (1 - self.alpha) * self.dist2.log_prob(z)
