function desc = vo_sift_cache(op, I, loc, d)
%VO_SIFT_CACHE descriptors of the last few libvo detections, keyed by image
%   (VO.m detects the left and the right image before it extracts either, VO.m:79-84).
%   loc is the N x 4 single key [Location, Scale, Orientation] of the points: keypoints with
%   several orientations share a Location.  'get' takes any subset or permutation of an entry's
%   rows (points = selectStrongest(points, N)) and returns their descriptors in that order.
    persistent entries
    desc = [];
    switch op
        case 'put'
            e = struct('I', I, 'loc', loc, 'desc', d);
            if isempty(entries)
                entries = e;
            else
                entries = [e, entries(1:min(end, 3))];
            end
        case 'get'
            for k = 1:numel(entries)
                if ~isequal(entries(k).I, I), continue; end
                [found, row] = ismember(loc, entries(k).loc, 'rows');
                if all(found)
                    desc = entries(k).desc(row, :);
                    return;
                end
            end
        case 'clear'
            entries = [];
    end
end
