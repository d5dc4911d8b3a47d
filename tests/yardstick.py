"""The project's measure for a float32 kernel against a float32 torch statement and the float64 evaluation of the same statement: TEST
INFRASTRUCTURE, shared by test_encode_edges.py and test_row_kernel_edges.py."""


def yardstick(name, got, r32, r64, where=None, loose_vs32=None, r64_for32=None, scaled=False, ratios=None):
    """The kernel is no further from the float64 value than 1.5 x the torch statement is (+1e-6 on the maximum, +1e-7 on the mean).  where: the
    elements it is applied to; the others (the i == j diagonal of dihedral-dependent tiles) are held to loose_vs32 x scale against the float32
    statement instead.  scaled: both floors are multiplied by max(1, max |float64 value|) of the tensor, as the flat tolerances of
    test_hip_parity.py scale theirs.  ratios: a dict that receives name -> (device error, float32 error) of the maximum.  Every figure is
    printed; -> the list of misses (the caller asserts it empty)."""
    assert got.shape == r64.shape == r32.shape, name
    e_hip, e_t32 = (got.double() - r64).abs(), (r32.double() - (r64 if r64_for32 is None else r64_for32)).abs()
    floor = max(1.0, r64.abs().max().item()) if scaled and r64.numel() else 1.0
    miss = []
    if where is not None:
        where = where.expand_as(e_hip)
        rest = (got - r32).abs()[~where]
        if rest.numel():
            scale = max(1.0, r64.abs().max().item())
            print(f'{name}: diagonal |hip - t32| {rest.max().item():.3e} bound {loose_vs32 * scale:.3e}')
            if not rest.max().item() <= loose_vs32 * scale:
                miss.append(f'{name}: diagonal {rest.max().item():.3e} > {loose_vs32 * scale:.3e}')
        e_hip, e_t32 = e_hip[where], e_t32[where]
    if e_hip.numel() == 0:
        return miss
    a, b, am, bm = e_hip.max().item(), e_t32.max().item(), e_hip.mean().item(), e_t32.mean().item()
    print(f'{name}: max hip {a:.3e} t32 {b:.3e}; mean hip {am:.3e} t32 {bm:.3e}' + (f'; floors x {floor:.3e}' if scaled else ''))
    if ratios is not None:
        ratios[name] = (a, b)
    if not a <= 1.5 * b + 1e-6 * floor:
        miss.append(f'{name}: max error {a:.3e} > 1.5 x {b:.3e} + {1e-6 * floor:.1e}')
    if not am <= 1.5 * bm + 1e-7 * floor:
        miss.append(f'{name}: mean error {am:.3e} > 1.5 x {bm:.3e} + {1e-7 * floor:.1e}')
    return miss
