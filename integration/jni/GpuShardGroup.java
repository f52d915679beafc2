package com.intel.distml.util.store;

import com.intel.distml.util.DataDesc;

/**
 * One PS process per GPU: shard `rank` of KeyRange.linearSplit(world)
 * (KeyRange.java:68-80) as an HBM-resident store, with device-resident
 * full-range pushes pre-reduced in push order, reduce-scattered over xGMI
 * (RCCL) and applied by their owner — include/distml_ps.h dml_group_*.
 * Rank 0 calls uniqueId() and the PS control plane (PSActor messages) hands the
 * 128 bytes to every rank before they construct their group.
 */
public class GpuShardGroup implements AutoCloseable {
    static { System.loadLibrary("distml_jni"); }

    private long handle;  // dml_group*
    private final int world;

    /** dml_group_pull's flag: records in the order of the key list instead of owner-major. */
    public static final int PULL_REQUEST_ORDER = 1;

    public static byte[] uniqueId() { return nativeUniqueId(); }

    public GpuShardGroup(byte[] uniqueId, int world, int rank, int device, DataDesc format,
                         long totalRows, int cols, int pieces) {
        this.world = world;
        handle = nativeGroupCreate(uniqueId, world, rank, device, format.dataType, format.keyType,
                format.valueType, format.denseRow ? 1 : 0, format.denseColumn ? 1 : 0,
                format.adaGrad ? 1 : 0, totalRows, cols, pieces);
    }

    /** Device pointers (HBM, this GPU) and byte lengths of up to 64 full-range pushes. */
    public void pushFullRange(long[] devPtrs, long[] lens) { nativeGroupPush(handle, devPtrs, lens, 0); }

    /**
     * Exact path for AdaGrad, int32-checked, array or key-subset pushes: split by owner
     * (SparseMatrix.push's per-partition split), exchanged with RCCL send/recv, applied by
     * each owner in rank-major push order. Every rank passes the same number of pushes.
     */
    public void pushExchange(long[] devPtrs, long[] lens) { nativeGroupPush(handle, devPtrs, lens, 1); }

    /** AdaGrad with many pushes per rank: Σu and Σu² reduce-scattered, within 1e-6 (not bit-exact). */
    public void pushMoments(long[] devPtrs, long[] lens) { nativeGroupPush(handle, devPtrs, lens, 2); }

    /**
     * Pushes the client already split to this shard (SparseMatrix.java:46-60): the exact
     * ordered apply, after every earlier call of this group. Push to storeHandle() directly
     * only after flush(): the group applies its calls in call order.
     */
    public void pushLocal(long[] devPtrs, long[] lens) { nativeGroupPush(handle, devPtrs, lens, 3); }

    /**
     * Order-exact path for float / double matrices, plain or AdaGrad: each shard's slice walks the ring
     * of ranks and every rank adds its own pushes' rows in push order, so shard s ends
     * byte-equal to a FloatMatrixStore / DoubleMatrixStore fed rank s's pushes, then rank
     * s+1's, ... (an arrival order PSAgent's selector may produce, PSAgent.java:166-186).
     * One model's bytes per rank over xGMI, whatever the number of pushes; ranks may pass
     * different numbers (0..64). An AdaGrad matrix (FloatMatrixStoreAdaGrad) ends with that
     * store's data, delta, alpha and maxDelta / maxDeltaRow / maxDeltaCol, byte for byte, with
     * one documented divergence: an element whose delta comes home NaN keeps the alpha its
     * owner held before the call (pushExchange is the path without it). int formats throw a
     * RuntimeException that names pushExchange's native call.
     */
    public void pushChained(long[] devPtrs, long[] lens) { nativeGroupPush(handle, devPtrs, lens, 4); }

    /**
     * The chained path for dense int matrices (IntMatrixStore, LightLDA's word-topic counts):
     * shard s ends equal to one IntMatrixStore fed rank s's pushes, then rank s+1's, ..., every
     * add checked (IntMatrixStore.java:154-178). A shard whose counter went negative holds the
     * adds up to that one, is closed for good, and its owner's next call or flush() throws the
     * IllegalStateException with the key and column; the other ranks' calls return normally
     * and the other shards go on. Other formats throw a RuntimeException naming pushChained's
     * native call.
     */
    public void pushChainedChecked(long[] devPtrs, long[] lens) { nativeGroupPush(handle, devPtrs, lens, 5); }

    /**
     * WorkerAgent.fetch (WorkerAgent.java:74-122) for key lists in HBM, a collective call: every
     * rank passes its own nkeys long keys at device address devKeys and receives their
     * handleFetch records at devOut (cap bytes) from the shards that own them, owner 0's
     * first, each in list order (the reference's byte[][] concatenated), or in list order with
     * PULL_REQUEST_ORDER. Keys outside the model are dropped. It sees every push call made
     * before it, with no flush() in between. Returns the number of records from every owner.
     */
    public long[] pull(long devKeys, long nkeys, long devOut, long cap, int flags) {
        java.nio.ByteBuffer b = java.nio.ByteBuffer.wrap(nativeGroupPull(handle, devKeys, nkeys, devOut, cap, flags, world))
                .order(java.nio.ByteOrder.LITTLE_ENDIAN);
        long[] counts = new long[world];
        for (int q = 0; q < world; ++q) counts[q] = b.getLong();
        return counts;
    }

    /** Every call applied; throws the first deferred key / repeated-row error. */
    public void flush() { nativeGroupFlush(handle); }

    /** dml_store* of this rank's shard (owned by the group), for fetch / checkpoint after flush(). */
    public long storeHandle() { return nativeGroupStore(handle); }

    public void close() {
        if (handle != 0) {
            nativeGroupDestroy(handle);
            handle = 0;
        }
    }

    private static native byte[] nativeUniqueId();
    private static native long nativeGroupCreate(byte[] id, int world, int rank, int device, int dataType,
                                                 int keyType, int valueType, int denseRow, int denseColumn,
                                                 int adaGrad, long totalRows, int cols, int pieces);
    private static native void nativeGroupPush(long g, long[] devPtrs, long[] lens, int mode);
    private static native byte[] nativeGroupPull(long g, long devKeys, long nkeys, long devOut, long cap, int flags,
                                                 int world);
    private static native void nativeGroupFlush(long g);
    private static native long nativeGroupStore(long g);
    private static native void nativeGroupDestroy(long g);
}
