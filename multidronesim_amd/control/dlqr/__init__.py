from .decentralized_lqr import DecentralizedLQR  # noqa: F401
