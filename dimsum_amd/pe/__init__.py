"""Positional encodings of DiM(pe_type=...): the module tree of the reference's dimsum/pe package on the HIP passes of ops/pos_embed.py."""
