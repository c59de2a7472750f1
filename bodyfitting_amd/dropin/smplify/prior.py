from bodyfitting_amd.prior import MaxMixturePrior  # noqa: F401
