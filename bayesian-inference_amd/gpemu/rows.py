"""Rows in blocks on the device: the one Python form of what ``RowsView`` (csrc/rows_dev.h) is in the library (DESIGN.md
§4.30).  Imports neither torch nor the library; ``columns`` does when it has to copy."""


class DeviceRows:
    """Rows of ``d`` doubles in the memory of ``device``, as ``n_blocks`` blocks of ``block_rows`` rows, the blocks
    ``block_stride_rows`` rows apart (a stored chain in place: a block is the walkers of one kept step): row r is at
    ``address + 8 d ((r // block_rows) block_stride_rows + r % block_rows)``.  ``stream``: the ``void *`` the rows were
    written on (waited for before they are read), or None.  ValueError for no block, an empty one, or overlapping ones."""

    def __init__(self, address, n_blocks, block_rows, block_stride_rows, stream=None, *, device=None, d=None):
        self.address, self.n_blocks, self.block_rows = int(address), int(n_blocks), int(block_rows)
        self.block_stride_rows, self.stream, self.device, self.d = int(block_stride_rows), stream, device, d
        self.rows = self.n_blocks * self.block_rows
        if self.n_blocks < 1 or self.block_rows < 1 or (self.n_blocks > 1 and self.block_stride_rows < self.block_rows):
            raise ValueError(f"bad block layout: {n_blocks} blocks of {block_rows} rows, {block_stride_rows} rows apart")

    @property
    def dense(self):
        """Is parameter j one stride, the rows one ``[rows][d]`` matrix?  The rule of ``RowsView::dense()`` in
        csrc/rows_dev.h; this is the one place it is written in Python."""
        return self.n_blocks == 1 or self.block_stride_rows == self.block_rows

    @property
    def layout(self):
        """The four numbers in the order every ``*_dev`` prototype of include/gpemu.h and every wrapper of one takes them."""
        return self.address, self.n_blocks, self.block_rows, self.block_stride_rows

    @classmethod
    def of_tensor(cls, x):
        """One dense block: the contiguous float64 device tensor ``x (S, d)``, which the result keeps alive."""
        out = cls(x.data_ptr(), 1, x.shape[0], x.shape[0], device=x.device.index or 0, d=int(x.shape[1]))
        out._tensor = x
        return out

    def columns(self):
        """These rows where ``dense``, else a dense ``[rows][d]`` copy made on torch's current stream, which the result owns."""
        if self.dense:
            return self
        import ctypes as C
        import torch
        from . import _lib
        x = torch.empty((self.rows, self.d), dtype=torch.float64, device=torch.device("cuda", self.device))
        _lib.check(_lib.lib().gpemu_marginal_dense_dev(self.device, C.c_void_p(self.address), *self.layout[1:], self.d,
                                                       C.c_void_p(x.data_ptr()), _lib.current_stream(self.device)))
        return DeviceRows.of_tensor(x)
