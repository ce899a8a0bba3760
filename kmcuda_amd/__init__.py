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
"""
from .api import kmeans_cuda, knn_cuda, supports_fp16  # noqa: F401
from .knn_index import KnnIndex, knn_query, knn_query_radius  # noqa: F401
from .predict import kmeans_predict, kmeans_predict_top  # noqa: F401
from .seed import kmeans_seed_parallel  # noqa: F401
from .minibatch import MiniBatchKMeans, kmeans_minibatch  # noqa: F401
