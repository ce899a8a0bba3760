"""kmcuda_amd -- MI355X (gfx950) native implementation of kmcuda's distance/assignment hot path.

Drop-in surface (mirrors the reference's `libKMCUDA` Python module, src/python.cc):
    from kmcuda_amd import kmeans_cuda, knn_cuda, supports_fp16
Step-level surface for row-sharded multi-process operation: kmcuda_amd.engine.Engine,
kmcuda_amd.distributed.
k-NN of new rows against a clustered corpus (beyond the reference): KnnIndex, knn_query; radius search on
the same index: KnnIndex.query_radius, knn_query_radius; multi-probe (approximate) search, only the nprobe nearest
clusters of every query or the clusters the caller lists: KnnIndex.query / knn_query with nprobe= or probes=.
A live index: KnnIndex.add takes more rows in place, KnnIndex.remove takes rows out of every later search (ids stay
stable, memory is not reclaimed); after either the index answers bit for bit as a freshly built one.
Filtered search: KnnIndex.query / knn_query with allow= (one flag per row id) answer a batch over a subset of the
corpus, exact or probed, bit for bit as an index without the other rows would, and leave the index as it is.
Masked radius search: KnnIndex.query_radius_allow / knn_query_radius with allow= -- query_radius's result with the
denied rows struck out, bit for bit.
Capped search: KnnIndex.query / knn_query with max_distance= return the k nearest rows within that distance, the cap
pruning from the first candidate on (exact, probed or masked); return_counts= appends the real entries per query.
New rows assigned to given centroids, with distances and cluster statistics (beyond the reference): kmeans_predict;
the m nearest centroids of every row, in the order an assignment pass would find them: kmeans_predict_top.
k-means|| seeding (beyond the reference), stand-alone -- kmeans_seed_parallel -- and as kmeans_cuda(init="k-means||").
Mini-batch K-means on a model that stays on the GPU (beyond the reference): MiniBatchKMeans (partial_fit, fit) and the
one-shot kmeans_minibatch.
Batched K-means over many small independent problems in one call (beyond the reference; product-quantiser codebooks
in place through a row stride): kmeans_batched, kmeans_predict_batched.
Top-k search over the uint8 product-quantiser codes those calls produce, by asymmetric distance computation (beyond
the reference): pq_search.
IVF-PQ (beyond the reference): codes of residuals in cluster lists, probed by the same ADC scan -- ivfpq_train,
IvfPqIndex (search), ivfpq_search on a caller's own lists.  The precomputed-term variant of that search (its own
bits, opt-in): ivfpq_terms, ivfpq_search(terms=), IvfPqIndex(precomputed=True).
4-bit codes, two to a byte, for both searches (the same definition in a sixteenth of the table): pq_pack4,
pq_search(bits=4), ivfpq_search(bits=4), IvfPqIndex(bits=4).
fp16 lookup tables for both byte-code searches (entries rounded once to binary16, summed in fp32: half the LDS, its
own bits, opt-in): pq_search(table_dtype="float16"), ivfpq_search(table_dtype="float16"),
IvfPqIndex(table_dtype="float16").
Non-residual IVF-PQ lists (the codes of the rows themselves: the table is pq_search's, built once per query and
copied by the scan blocks; opt-in): ivfpq_train(residual=False), IvfPqIndex(residual=False),
ivfpq_search(residual=False).
Exact re-ranking of per-query candidate lists against the raw rows, the step behind such a shortlist (beyond the
reference): knn_rerank, and IvfPqIndex(keep_rows=True).search(refine=).
"""
from .api import kmeans_cuda, knn_cuda, supports_fp16  # noqa: F401
from .knn_index import KnnIndex, knn_query, knn_query_radius  # noqa: F401
from .predict import kmeans_predict, kmeans_predict_top  # noqa: F401
from .seed import kmeans_seed_parallel  # noqa: F401
from .minibatch import MiniBatchKMeans, kmeans_minibatch  # noqa: F401
from .batched import kmeans_batched, kmeans_predict_batched  # noqa: F401
from .pq import pq_pack4, pq_search  # noqa: F401
from .ivfpq import IvfPqIndex, ivfpq_search, ivfpq_terms, ivfpq_train, knn_rerank  # noqa: F401
