"""Evaluation protocols that run on this project's own kernels (instance_level: the Cityscapes instance-level AP)."""
